"""The layers behind the attention: the back half of the reference's DynEnvFeatureExtractor.forward (DynEnv/models/models.py:584-594,
610-616; LSTMLayer: models.py:16-95) - TransformNet, the LSTM cell on its persistent state, the closing LayerNorm - differentiable
through torch where a gradient is wanted and ONE kernel (dynenv_recurrent_head, csrc/recurrent_kernels.hip) where none is; and the whole
extractor composed of the three device layers under the reference's parameter names."""
import ctypes as C
import os

from . import _capi

# torch is imported on first use (the package itself imports without it): the nn.Modules are built then.
_lazy = {}


def _classes():
    if "rec" not in _lazy:
        import torch
        nn = torch.nn

        class _Lstm(nn.Module):
            """the parameters of the reference's LSTMLayer under its names: cell and transformer (the state lives in the head)"""

            def __init__(self, feature_size, device=None):
                super().__init__()
                self.cell = nn.LSTMCell(feature_size, feature_size, device=device)
                self.transformer = nn.Sequential(nn.Linear(6, feature_size, device=device), nn.Tanh())

        class GpuRecurrentHead(nn.Module):
            """The tail of the reference's DynEnvFeatureExtractor, parameter for parameter and name for name - TransformNet:
            Sequential(Linear(F + X, F), LeakyReLU(0.1), LayerNorm(F)); LSTM: cell = nn.LSTMCell(F, F) and transformer =
            Sequential(Linear(6, F), Tanh()); bn: LayerNorm(F) - so that those keys of a DynEnvFeatureExtractor.state_dict() load with
            strict=True.  forward(features, position=None, reset_env=None) -> [P, F], P = num_players * num_envs, row p of environment
            p // num_players (the arranger's player order): models.py:610-616 on `features`, what GpuTemporalAttention returns.

            STATE.  `h` and `c` [P, F] are plain attributes as in the reference's LSTMLayer, not buffers: state_dict() holds parameters
            alone.  reset(reset_indices=None) zeroes every environment whatever reset_indices says, detach(), get_states(),
            set_states(states) and set_state(locInits) behave as the reference's (models.py:40-75).  Two differences: reset zeroes IN
            PLACE - two fixed tensors, no reallocation - and reset_envs(mask) zeroes the rows of the environments listed in a bool /
            uint8 [num_envs] device tensor on the device, nothing read on the host.  forward's reset_env= takes the same mask and
            applies the same reset before the cell - a step's `dones` tensor is one.

            Routes; `last_route` names the one the latest forward took.
              "torch"  when gradients are enabled and a parameter requires one: the reference's operations in order, differentiable;
                       `h` and `c` are rebound to the cell's results as the reference does (reset_env= through torch.where).
              "fused"  otherwise: one launch.  The state lives in two module-owned fixed tensors that the kernel updates in place; if
                       `h` / `c` are not those (after a torch-route call or set_states) they are first copied in on the stream and
                       rebound, so the pointers never change and the call captures.  The reset is folded into the kernel: the state of
                       a listed environment is not read.  It takes F of 64 or 128, X <= 32, float32 contiguous inputs and parameters
                       on the device.  The 16-bit copies of the three weight matrices (operand_dtype, TransformNet's zero-padded to a
                       multiple of 32 columns) are made with torch ops on the stream at every call: no host wait.
              "torch (fallback: ...)"  where no gradient is wanted but the kernel does not take the call - another F, X > 32, a
                       `position` of another width than X, inputs or parameters that are not float32 and contiguous, a CPU device,
                       DYNENV_RHEAD_FUSED=0 in the environment.  Nothing is raised.
            ARITHMETIC of the fused route: 16-bit operands on the matrix units, float32 accumulation; biases, LeakyReLU, the LayerNorms,
            the gates and the state in float32 (c is never rounded) - the torch route under torch.autocast."""

            def __init__(self, feature_size, num_players, num_envs, extended_feature_cnt=0, operand_dtype=torch.bfloat16, device=None):
                super().__init__()
                F, X = int(feature_size), int(extended_feature_cnt)
                self.feature_size, self.extended_feature_cnt = F, X
                self.num_players, self.num_envs = int(num_players), int(num_envs)
                self.operand_dtype = operand_dtype
                assert self.operand_dtype in (torch.bfloat16, torch.float16), "operand_dtype is torch.bfloat16 or torch.float16"
                self.TransformNet = nn.Sequential(nn.Linear(F + X, F, device=device), nn.LeakyReLU(0.1), nn.LayerNorm(F, device=device))
                self.hidden_size = F
                self.LSTM = _Lstm(F, device=device)
                self.bn = nn.LayerNorm(F, device=device)
                self._fixed = None
                self._route = None
                w = self.LSTM.cell.weight_ih
                self.h = torch.zeros((self.num_players * self.num_envs, F), dtype=w.dtype, device=w.device)
                self.c = torch.zeros_like(self.h)

            @property
            def last_route(self):
                return self._route

            # ---- the state (models.py:40-89)
            def _fixed_state(self):
                """the two module-owned tensors of the parameters' type and device, made once"""
                w = self.LSTM.cell.weight_ih
                if self._fixed is None or self._fixed[0].dtype != w.dtype or self._fixed[0].device != w.device:
                    shape = (self.num_players * self.num_envs, self.hidden_size)
                    self._fixed = (torch.zeros(shape, dtype=w.dtype, device=w.device), torch.zeros(shape, dtype=w.dtype, device=w.device))
                return self._fixed

            @staticmethod
            def _same(a, b):
                return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype and a.device == b.device and a.is_contiguous()

            def _state_into_fixed(self):
                hb, cb = self._fixed_state()
                with torch.no_grad():
                    if not self._same(self.h, hb):
                        hb.copy_(self.h)
                    if not self._same(self.c, cb):
                        cb.copy_(self.c)
                self.h, self.c = hb, cb
                return hb, cb

            def reset(self, reset_indices=None):
                """every environment's state to zero, whatever reset_indices says (the reference's, models.py:40-55) - in place"""
                hb, cb = self._fixed_state()
                with torch.no_grad():
                    hb.zero_()
                    cb.zero_()
                self.h, self.c = hb, cb

            def _rows(self, mask):
                E, A = self.num_envs, self.num_players
                assert tuple(mask.shape) == (E,), "a reset mask is bool / uint8 [num_envs]"
                return mask.bool().view(E, 1).expand(E, A).reshape(E * A, 1)

            def reset_envs(self, mask):
                """the rows of the environments listed in `mask` (bool / uint8 [num_envs], on the state's device) to zero, on the device"""
                rows = self._rows(mask)
                with torch.no_grad():
                    if self.h.grad_fn is None and self.c.grad_fn is None:
                        self.h.masked_fill_(rows, 0)
                        self.c.masked_fill_(rows, 0)
                    else:
                        self.h, self.c = self.h.masked_fill(rows, 0), self.c.masked_fill(rows, 0)

            def detach(self):
                self.h = self.h.detach()
                self.c = self.c.detach()

            def get_states(self):
                return [self.h.clone(), self.c.clone()]

            def set_states(self, states):
                self.h = states[0].clone()
                self.c = states[1].clone()

            def set_state(self, state):
                x = state.to(self.LSTM.cell.weight_ih.device)
                self.c = self.LSTM.transformer(x)
                self.f = self.c

            def _apply(self, fn, *args, **kwargs):
                super()._apply(fn, *args, **kwargs)
                self.h, self.c = fn(self.h), fn(self.c)
                self._fixed = None
                return self

            # ---- forward
            def _not_fusable(self, features, position, reset_env):
                """why the kernel does not take this call, or None"""
                F, X, P = self.feature_size, self.extended_feature_cnt, self.num_players * self.num_envs
                if os.environ.get("DYNENV_RHEAD_FUSED", "") == "0":
                    return "DYNENV_RHEAD_FUSED=0"
                if F not in (64, 128):
                    return "F = %d, not 64 or 128" % F
                if X > 32:
                    return "X = %d, above 32" % X
                if not features.is_cuda:
                    return "features that are not on the device"
                if position is not None and (position.dim() != 2 or position.shape[1] != X or X == 0):
                    return "a position of width %s, not X = %d" % (position.shape[1] if position.dim() == 2 else "?", X)
                tensors = [features, self.h, self.c] + ([position] if position is not None else [])
                for t, cols in zip(tensors, [F, F, F, X]):
                    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (P, cols) or t.device != features.device:
                        return "inputs or a state that are not float32, contiguous [%d, .] and on %s" % (P, features.device)
                if reset_env is not None and (reset_env.dtype not in (torch.bool, torch.uint8) or tuple(reset_env.shape) != (self.num_envs,)
                                              or not reset_env.is_contiguous() or reset_env.device != features.device):
                    return "a reset_env that is not bool / uint8 [%d] on %s" % (self.num_envs, features.device)
                for p in self._head_parameters():
                    if p.dtype != torch.float32 or not p.is_contiguous() or p.device != features.device:
                        return "parameters that are not float32, contiguous and on %s" % (features.device,)
                return None

            def _head_parameters(self):
                return list(self.TransformNet.parameters()) + list(self.LSTM.parameters()) + list(self.bn.parameters())

            def forward(self, features, position=None, reset_env=None):
                return self._head(features, position, reset_env)

            def _head(self, features, position, reset_env):
                if torch.is_grad_enabled() and any(p.requires_grad for p in self._head_parameters()):
                    self._route = "torch"
                    return self._forward_torch(features, position, reset_env)
                why = self._not_fusable(features, position, reset_env)
                if why is not None:
                    self._route = "torch (fallback: %s)" % why
                    return self._forward_torch(features, position, reset_env)
                self._route = "fused"
                return self._forward_fused(features, position, reset_env)

            def _forward_torch(self, features, position, reset_env):
                """models.py:610-616 and 92-95 line for line; the reset through torch.where"""
                if position is not None:
                    features = self.TransformNet(torch.cat((features, position), dim=1))
                h, c = self.h, self.c
                if reset_env is not None:
                    rows = self._rows(reset_env)
                    h, c = torch.where(rows, torch.zeros_like(h), h), torch.where(rows, torch.zeros_like(c), c)
                self.h, self.c = self.LSTM.cell(features, (h, c))
                return self.bn(self.h)

            def _forward_fused(self, features, position, reset_env):
                F, X, E, A = self.feature_size, self.extended_feature_cnt, self.num_envs, self.num_players
                dev, dt = features.device, self.operand_dtype
                h, c = self._state_into_fixed()
                out = torch.empty((E * A, F), dtype=torch.float32, device=dev)
                cell, lin, tln = self.LSTM.cell, self.TransformNet[0], self.TransformNet[2]
                # the 16-bit operands: alive until the launch is enqueued (the caching allocator orders their reuse on the stream)
                keep = [cell.weight_ih.detach().to(dt), cell.weight_hh.detach().to(dt)]
                w = _capi.Rhead()
                if position is not None:
                    KP = (F + X + 31) // 32 * 32
                    tr = torch.zeros((F, KP), dtype=dt, device=dev)
                    tr[:, :F + X] = lin.weight.detach()
                    keep.append(tr)
                    w.tr_w, w.tr_b, w.tr_ln_w, w.tr_ln_b = tr.data_ptr(), lin.bias.data_ptr(), tln.weight.data_ptr(), tln.bias.data_ptr()
                w.w_ih, w.w_hh = keep[0].data_ptr(), keep[1].data_ptr()
                w.b_ih, w.b_hh, w.ln_w, w.ln_b = cell.bias_ih.data_ptr(), cell.bias_hh.data_ptr(), self.bn.weight.data_ptr(), self.bn.bias.data_ptr()
                mask = None
                if reset_env is not None:
                    mask = reset_env.view(torch.uint8) if reset_env.dtype == torch.bool else reset_env
                lib = _capi.load()
                with torch.cuda.device(dev):
                    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    _capi.check(lib.dynenv_recurrent_head(_capi.ptr(features), _capi.ptr(position), E, A, F, X if position is not None else 0,
                                                          1 if dt == torch.bfloat16 else 2, C.byref(w), float(self.TransformNet[1].negative_slope),
                                                          float(tln.eps), float(self.bn.eps), _capi.ptr(mask), _capi.ptr(h), _capi.ptr(c),
                                                          _capi.ptr(out), stream), "dynenv_recurrent_head")
                return out

        class GpuFeatureExtractor(GpuRecurrentHead):
            """The reference's DynEnvFeatureExtractor (models.py:574-619) of the three device layers, under its parameter names: InNet =
            GpuEmbedInputLayer(types, feature_size, nEnvs, nAgents, nTime, obs_dim, fixed, padded_dtype), AttNet =
            GpuTemporalAttention(feature_size), and GpuRecurrentHead's TransformNet, LSTM and bn at top level - a
            DynEnvFeatureExtractor.state_dict() loads with strict=True.  forward(obs, position=None, count_env=None, reset_env=None) ->
            [nEnvs * nAgents, F] is models.py:603-619 on the dense observation tensor; reset, detach and the state are the head's.
            `last_route` is the three layers' routes (InNet's, AttNet's, the head's).  The head's operands take padded_dtype where that
            is torch.float16, bfloat16 otherwise."""

            def __init__(self, types, feature_size, nEnvs, nAgents, nTime, obs_dim, extended_feature_cnt=0, fixed=None, padded_dtype=None):
                from .arranger import GpuEmbedInputLayer
                from .attention import GpuTemporalAttention
                # (the input layer first: it decides the device)
                in_net = GpuEmbedInputLayer(types, feature_size, nEnvs, nAgents, nTime, obs_dim, fixed=fixed, padded_dtype=padded_dtype)
                dev = in_net.arranger.device
                GpuRecurrentHead.__init__(self, feature_size, nAgents, nEnvs, extended_feature_cnt,
                                          operand_dtype=torch.float16 if padded_dtype == torch.float16 else torch.bfloat16, device=dev)
                self.InNet = in_net
                self.AttNet = GpuTemporalAttention(feature_size, device=dev)
                for k in ("TransformNet", "LSTM", "bn"):   # (the reference's order of members, so also of state_dict())
                    self._modules[k] = self._modules.pop(k)

            @property
            def last_route(self):
                return (self.InNet.last_route, self.AttNet.last_route, self._route)

            def forward(self, obs, position=None, count_env=None, reset_env=None):
                x = self.InNet(obs, count_env)
                counts = self.InNet.last_obj_counts if self.InNet.last_route == "fused" else None
                features = self.AttNet(x, counts)
                return self._head(features, position, reset_env)

        GpuRecurrentHead.__qualname__, GpuFeatureExtractor.__qualname__ = "GpuRecurrentHead", "GpuFeatureExtractor"
        _lazy["rec"] = {"GpuRecurrentHead": GpuRecurrentHead, "GpuFeatureExtractor": GpuFeatureExtractor}
    return _lazy["rec"]


def __getattr__(name):
    if name in ("GpuRecurrentHead", "GpuFeatureExtractor"):
        return _classes()[name]
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
