"""GPU-side ragged -> padded arranger: the host mirror of the reference's `InOutArranger`
(DynEnv/models/models.py:208-274) over the dense observation tensor `BatchedDynEnv.step_flat()` returns.

The reference's input layer does, per forward pass, in triple-nested Python over object arrays:
    inputs, counts = arranger.rearrange_inputs(x)                  # x = obs[..., g], ragged lists
    outs = [block(torch.tensor(obj)) for block, obj in zip(blocks, inputs)]
    outs, masks = arranger.rearrange_outputs(outs, counts, device)
Here the same three calls exist with the same results, but `x` is the dense device tensor and all index work runs in the
HIP kernels of `csrc/arranger_kernels.hip` through the C ABI (`dynenv_arrange_*`, include/dynenv.h).  No CPU fallback.
"""
import ctypes as C
import os

from . import _capi
from .obs_layout import row_groups


def groups_for(env):
    """The object-type groups of an environment's observation, as the reference splits them into obs[..., 0] (movable
    objects) and obs[..., 1] (self / static rows); see obs_layout.row_groups.
    Returns {"movable": [ArrType...], "static": [ArrType...]}."""
    groups = row_groups(env.layout, env.env_type, env.observationType)
    return {name: [_capi.ArrType(*ty, 0) for ty in groups[name]] for name in ("movable", "static")}


class GpuInOutArranger(object):
    """Same role and call sequence as the reference's InOutArranger(nObjectTypes, nPlayers, nTime) (models.py:208-216);
    `nPlayers` is E*A as in InputLayer (:283).  `types` describes where each object type lives in an observation row."""

    def __init__(self, types, nEnvs, nAgents, nTime, obs_dim, device=None):
        import torch
        if not torch.cuda.is_available():
            raise _capi.DynEnvError("dynenv_amd needs an MI355X (HIP device); there is no CPU fallback")
        self._torch = torch
        self._lib = _capi.load()
        self.nObjectTypes = len(types)
        if not 1 <= self.nObjectTypes <= _capi.ARR_MAX_TYPES:
            raise ValueError("1..%d object types per group" % _capi.ARR_MAX_TYPES)
        self.types = (_capi.ArrType * self.nObjectTypes)(*types)
        self.E, self.A, self.nTime, self.D = int(nEnvs), int(nAgents), int(nTime), int(obs_dim)
        self.nPlayers = self.E * self.A
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        TP = self.nTime * self.nPlayers
        i32 = dict(dtype=torch.int32, device=self.device)
        self._counts = torch.empty((self.nObjectTypes, self.nTime, self.nPlayers), **i32)
        self._obj_counts = torch.empty((self.nTime, self.nPlayers), **i32)
        self._base = torch.empty((self.nObjectTypes, self.nTime, self.nPlayers), **i32)
        n = int(self._lib.dynenv_arrange_scratch_ints(self.E, self.nTime, self.A, self.nObjectTypes))
        self._scratch = torch.empty((n + 2,), **i32)
        self.feats = [int(t.feat) for t in types]

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def rearrange_inputs(self, obs, count_env=None):
        """obs: dense float32 device tensor [E, T, A, D]; count_env: int32 [E, 2] from BatchedDynEnv.counts() when a type
        counts per environment.  Returns (inputs, (counts, maxCount, objCounts, slots)) like models.py:219-250:
        inputs[i] float32 [N_i, feat_i] in (time, player, object) order; counts int32 [type, T, P]; objCounts [T, P]."""
        torch = self._torch
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous()
        assert tuple(obs.shape) == (self.E, self.nTime, self.A, self.D), (tuple(obs.shape), (self.E, self.nTime, self.A, self.D))
        plan = _capi.ArrPlan()
        _capi.check(self._lib.dynenv_arrange_plan(_capi.ptr(obs), self.E, self.nTime, self.A, self.D, self.types,
                                                  self.nObjectTypes, _capi.ptr(count_env), _capi.ptr(self._counts),
                                                  _capi.ptr(self._obj_counts), _capi.ptr(self._base), _capi.ptr(self._scratch),
                                                  C.byref(plan), self._stream()), "dynenv_arrange_plan")
        max_count = int(plan.max_count)
        inputs = [torch.empty((int(plan.total[i]), self.feats[i]), dtype=torch.float32, device=self.device)
                  for i in range(self.nObjectTypes)]
        slots = [torch.empty((int(plan.total[i]),), dtype=torch.int32, device=self.device) for i in range(self.nObjectTypes)]
        mask = torch.empty((self.nTime, self.nPlayers, max_count), dtype=torch.uint8, device=self.device)
        vp = C.c_void_p
        in_ptrs = (vp * self.nObjectTypes)(*[t.data_ptr() if t.numel() else None for t in inputs])
        sl_ptrs = (vp * self.nObjectTypes)(*[t.data_ptr() if t.numel() else None for t in slots])
        _capi.check(self._lib.dynenv_arrange_gather(_capi.ptr(obs), self.E, self.nTime, self.A, self.D, self.types,
                                                    self.nObjectTypes, _capi.ptr(self._counts), _capi.ptr(self._base), max_count,
                                                    in_ptrs, sl_ptrs, _capi.ptr(mask) if max_count else vp(0), self._stream()),
                    "dynenv_arrange_gather")
        return inputs, (self._counts, max_count, self._obj_counts, slots, mask)

    def rearrange_outputs(self, outs, countArr, device=None):
        """outs[i]: float32 [N_i, F] embeddings of inputs[i] (or None).  Returns (padded [T, maxCount, P, F],
        masks = list over time of bool [P, maxCount]) like models.py:252-274."""
        torch = self._torch
        _, max_count, _, slots, mask = countArr
        if len(outs) != self.nObjectTypes:
            raise ValueError("rearrange_outputs: %d outputs for %d object types" % (len(outs), self.nObjectTypes))
        # a type without any object has out = None in the reference (:262); its counts are all zero, so it shifts nothing.
        # None for a type WITH objects would make the reference pack the later types to the left (:259-266) where the kernels
        # leave a gap of zeros: refused.
        for i, o in enumerate(outs):
            if o is None and int(slots[i].shape[0]):
                raise ValueError("rearrange_outputs: outs[%d] is None but object type %d has %d objects"
                                 % (i, i, int(slots[i].shape[0])))
        F = next(int(o.shape[1]) for o in outs if o is not None)
        ok = F % 4 == 0 and all(o is None or (o.is_cuda and o.dtype == torch.float32 and o.is_contiguous() and
                                              o.shape[1] == F and o.data_ptr() % 16 == 0) for o in outs)
        n_obj = sum(int(o.shape[0]) for o in outs if o is not None)
        # One pass over the padded tensor (5.4-5.7 TB/s on MI355X) unless it is almost all padding: below ~6 % occupancy a memset
        # (7 TB/s) + a scatter of the few rows moves less (driving Partial at 19 %: 0.150 ms in one pass against 0.196 ms).
        dense = n_obj >= float(os.environ.get('DYNENV_ARR_DENSE_MIN', '0.06')) * self.nTime * max_count * self.nPlayers
        if ok and dense:  # one pass over the padded tensor, padding zeros included
            padded = torch.empty((self.nTime, max_count, self.nPlayers, F), dtype=torch.float32, device=self.device)
            vp = C.c_void_p
            ptrs = (vp * self.nObjectTypes)(*[o.data_ptr() if (o is not None and o.shape[0]) else None for o in outs])
            _capi.check(self._lib.dynenv_arrange_pad(ptrs, _capi.ptr(self._counts), _capi.ptr(self._base), self.nObjectTypes,
                                                     self.nTime, self.nPlayers, max_count, F, _capi.ptr(padded),
                                                     self._stream()), "dynenv_arrange_pad")
        else:  # odd widths: zero fill + one scatter per type
            padded = torch.zeros((self.nTime, max_count, self.nPlayers, F), dtype=torch.float32, device=self.device)
            for i, out in enumerate(outs):
                if out is None or out.shape[0] == 0:
                    continue
                out = out.contiguous().float()
                _capi.check(self._lib.dynenv_arrange_scatter(_capi.ptr(out), _capi.ptr(slots[i]), int(out.shape[0]), F,
                                                             _capi.ptr(padded), self._stream()), "dynenv_arrange_scatter")
        masks = [mask[t].bool() for t in range(self.nTime)]
        return padded, masks
