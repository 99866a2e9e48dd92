"""The layer behind the input layer: the reference's RecurrentTemporalAttention (DynEnv/models/models.py:311-386) over the padded tensor,
differentiable through torch where a gradient is wanted and ONE kernel (dynenv_attend_pool, csrc/attention_kernels.hip) where none is."""
import ctypes as C
import os

from . import _capi

# torch is imported on first use (the package itself imports without it): the nn.Module is built then.
_lazy = {}


def _attention_class():
    if "att" not in _lazy:
        import torch
        nn = torch.nn

        class GpuTemporalAttention(nn.Module):
            """The reference's RecurrentTemporalAttention (models.py:311-386), parameter for parameter and name for name - objAtt and
            tempAtt: nn.MultiheadAttention(F, num_heads, add_bias_kv=True); bn: LayerNorm(F); confLayer: Sequential(Linear(F, 1),
            Sigmoid()) - so that a RecurrentTemporalAttention.state_dict() loads with strict=True.
            forward(x, obj_counts=None) -> [P, F], x = (padded [T, M, P, F], masks) exactly as GpuInputLayer / GpuEmbedInputLayer return
            it; obj_counts an optional int32 [T, P] device tensor (GpuEmbedInputLayer.last_obj_counts) - without it the counts are
            M - mask.sum(1), taken on the device.

            Two routes; `last_route` names the one the latest forward took.
              "torch"  when gradients are enabled and a parameter requires one: the reference's forward restated in torch - the same
                       operations in the same order, differentiable - without its three prints and their .any() host reads, and with
                       the NaN filter written as torch.where(isnan, 0, att): nothing is read on the host, so it can be captured.
              "fused"  otherwise: one launch from the padded tensor and the counts to [P, F] float32.  It takes num_heads == 1, F of 64
                       or 128, M <= 128, `padded` contiguous on the device in bfloat16 or float16, float32 contiguous parameters on that
                       device.  The 16-bit copies of the four weight matrices and the bias_k / bias_v rows are made with torch ops on
                       the stream at every call: no host wait, so the call captures.  THE MASKS ARE TAKEN AS PREFIXES (True from the
                       count on), which the arranger's are: a slot at or behind a player's count is never read.
              "torch (fallback: ...)"  where no gradient is wanted but the kernel does not take the call - a float32 `padded`, another
                       F, M > 128, more heads, DYNENV_ATT_FUSED=0 in the environment, a CPU device.  Nothing is raised.  One shape the
                       kernel takes goes this way by MEASUREMENT: M = 1 at F = 128 (RoboCup Full's static group), where the kernel's
                       fixed cost per player - it streams the weights once per player - exceeded the torch route's 1.4 times at 4096
                       environments (profiles/HISTORY.md); DYNENV_ATT_FUSED=1 takes the kernel wherever it can run.
            ARITHMETIC of the fused route: 16-bit operands on the matrix units, float32 accumulation; biases, softmax, LayerNorm, sigmoid
            and the mean in float32 - the torch route under torch.autocast, with a rounding fewer between some products."""

            def __init__(self, feature_size, num_heads=1, device=None):
                super().__init__()
                self.feature_size = int(feature_size)
                self.num_heads = int(num_heads)
                self.objAtt = nn.MultiheadAttention(feature_size, num_heads, add_bias_kv=True, device=device)
                self.tempAtt = nn.MultiheadAttention(feature_size, num_heads, add_bias_kv=True, device=device)
                self.bn = nn.LayerNorm(feature_size, device=device)
                self.confLayer = nn.Sequential(nn.Linear(feature_size, 1, device=device), nn.Sigmoid())
                self.last_route = None

            def _not_fusable(self, padded):
                """why the kernel does not take this call, or None"""
                env = os.environ.get("DYNENV_ATT_FUSED", "")
                if env == "0":
                    return "DYNENV_ATT_FUSED=0"
                if self.num_heads != 1:
                    return "num_heads = %d, not 1" % self.num_heads
                if self.feature_size not in (64, 128):
                    return "F = %d, not 64 or 128" % self.feature_size
                if not padded.is_cuda:
                    return "a padded tensor that is not on the device"
                if padded.dtype not in (torch.bfloat16, torch.float16):
                    return "a padded tensor of %s, not bfloat16 or float16" % str(padded.dtype).replace("torch.", "")
                if padded.dim() != 4 or padded.shape[3] != self.feature_size or not padded.is_contiguous():
                    return "a padded tensor that is not contiguous [T, M, P, %d]" % self.feature_size
                if padded.shape[1] > 128:
                    return "M = %d, above 128" % padded.shape[1]
                if padded.shape[0] < 1 or padded.shape[2] < 1:
                    return "an empty batch"
                if padded.shape[1] == 1 and self.feature_size == 128 and env != "1":
                    # (the one measured shape the kernel loses at - RoboCup Full's static group, the self row alone: profiles/HISTORY.md)
                    return "M = 1 at F = 128, where the torch route measured faster (DYNENV_ATT_FUSED=1 takes the kernel)"
                for p in self.parameters():
                    if p.dtype != torch.float32 or not p.is_contiguous() or p.device != padded.device:
                        return "parameters that are not float32, contiguous and on %s" % (padded.device,)
                return None

            def forward(self, x, obj_counts=None):
                if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
                    self.last_route = "torch"
                    return self._forward_torch(x)
                why = self._not_fusable(x[0])
                if why is not None:
                    self.last_route = "torch (fallback: %s)" % why
                    return self._forward_torch(x)
                self.last_route = "fused"
                return self._forward_fused(x, obj_counts)

            def _forward_torch(self, x):
                """models.py:332-386 line for line, less the prints; index assignments through a mask (which count the mask's elements on
                the host) are written as where / masked_fill / clamp, which give the same values"""
                tensor, masks = x
                if tensor.dtype != self.bn.weight.dtype and not torch.is_autocast_enabled(tensor.device.type):
                    tensor = tensor.to(self.bn.weight.dtype)   # (outside autocast a Linear wants its parameters' type: a 16-bit padded tensor is widened)
                attObj = []
                for objs, mask in zip(tensor, masks):
                    att = self.objAtt(objs, objs, objs, mask)[0]
                    attObj.append(torch.where(torch.isnan(att), torch.zeros_like(att), att))
                finalAtt = attObj[0]
                finalMask = masks[0]
                for i in range(0, len(attObj) - 1):
                    temp = self.bn(self.tempAtt(attObj[i + 1], finalAtt, finalAtt, finalMask)[0])
                    finalMask = masks[i + 1] & finalMask
                    finalAtt = torch.where(torch.isnan(temp), torch.zeros_like(temp), temp)
                finalMask = finalMask.permute(1, 0)
                finalAtt = finalAtt.masked_fill(finalMask.unsqueeze(2), 0)
                if finalAtt.shape[0] == 0:
                    return torch.sum(finalAtt, 0)
                confs = self.confLayer(finalAtt)
                summed = torch.sum(finalAtt * confs, 0)
                lens = torch.sum(torch.logical_not(finalMask), 0).float().unsqueeze(1)
                return summed.div(lens.clamp(min=1.0))

            def _forward_fused(self, x, obj_counts):
                padded, masks = x
                T, M, P, F = (int(s) for s in padded.shape)
                dev, dt = padded.device, padded.dtype
                if obj_counts is None:
                    if M:
                        obj_counts = (M - torch.stack(list(masks)).sum(2)).to(torch.int32)
                    else:
                        obj_counts = torch.zeros((T, P), dtype=torch.int32, device=dev)
                assert obj_counts.is_cuda and obj_counts.dtype == torch.int32 and obj_counts.is_contiguous() and tuple(obj_counts.shape) == (T, P)
                out = torch.empty((P, F), dtype=torch.float32, device=dev)
                keep = []   # the 16-bit operands: alive until the launch is enqueued (the caching allocator orders their reuse on the stream)

                def mha(m):
                    w16 = [m.in_proj_weight.detach().to(dt), m.out_proj.weight.detach().to(dt), m.bias_k.detach().to(dt).reshape(F),
                           m.bias_v.detach().to(dt).reshape(F)]
                    keep.extend(w16)
                    return _capi.Mha(*[t.data_ptr() for t in w16 + [m.in_proj_bias, m.out_proj.bias]])

                obj, tmp = mha(self.objAtt), mha(self.tempAtt)
                lin = self.confLayer[0]
                lib = _capi.load()
                with torch.cuda.device(dev):
                    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    _capi.check(lib.dynenv_attend_pool(_capi.ptr(padded) if M else None, 1 if dt == torch.bfloat16 else 2, _capi.ptr(obj_counts), T, M, P, F,
                                                       C.byref(obj), C.byref(tmp), _capi.ptr(self.bn.weight), _capi.ptr(self.bn.bias), float(self.bn.eps),
                                                       _capi.ptr(lin.weight), _capi.ptr(lin.bias), _capi.ptr(out), stream), "dynenv_attend_pool")
                return out

        GpuTemporalAttention.__qualname__ = "GpuTemporalAttention"
        _lazy["att"] = GpuTemporalAttention
    return _lazy["att"]


def __getattr__(name):
    if name == "GpuTemporalAttention":
        return _attention_class()
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
