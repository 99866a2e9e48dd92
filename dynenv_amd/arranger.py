"""GPU-side ragged -> padded arranger: the host mirror of the reference's `InOutArranger`
(DynEnv/models/models.py:208-274) over the dense observation tensor `BatchedDynEnv.step_flat()` returns.

The reference's input layer does, per forward pass, in triple-nested Python over object arrays:
    inputs, counts = arranger.rearrange_inputs(x)                  # x = obs[..., g], ragged lists
    outs = [block(torch.tensor(obj)) for block, obj in zip(blocks, inputs)]
    outs, masks = arranger.rearrange_outputs(outs, counts, device)
Here the same three calls exist with the same results, but `x` is the dense device tensor and all index work runs in the
HIP kernels of `csrc/arranger_kernels.hip` and `csrc/arranger_cols_kernels.hip` through the C ABI (`dynenv_arrange_*`,
include/dynenv.h).  No CPU fallback.

Like the reference's (out[range] -> torch.cat -> F.pad -> torch.stack, models.py:250-274), `rearrange_outputs` is differentiable:
the embedding blocks train through it (a torch.autograd.Function over `dynenv_arrange_pad_backward` /
`dynenv_arrange_scatter_backward`).  `GpuInputLayer` is the three calls as one nn.Module.

Two modes.  The default pads to the largest object count of each batch, as the reference does, and so has to wait for the device to
learn the shapes.  `fixed=...` works at capacities the caller fixes once (`dynenv_arrange_fixed_*`, csrc/arranger_fixed_kernels.hip and
the fixed-mode kernels of csrc/arranger_cols_kernels.hip): the same layout in the leading slots, zeros behind, no host round trip,
capturable into a graph.

In both modes `padded_dtype=torch.bfloat16` (or float16) writes the padded tensor in that type, for a network under torch.autocast
(`dynenv_arrange_*_as`, csrc/arranger_cols_kernels.hip): float32 embeddings are converted on the way (round to nearest even), embeddings
already of that type are copied bit for bit, and the backward hands every embedding a gradient of its own type.

`GpuEmbedInputLayer` is the reference's whole InputLayer (models.py:278-307), its EmbedBlocks (:99-124) included: the three calls above
when a gradient is wanted, and otherwise ONE kernel from the observation rows to the padded tensor (`dynenv_arrange_embed_pad`,
csrc/arranger_embed_kernels.hip) - no inputs[i], no activation and no embedding is written or read back.
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

    def __init__(self, types, nEnvs, nAgents, nTime, obs_dim, device=None, fixed=None, padded_dtype=None):
        """fixed=None: the reference's shapes - every call pads to the largest object count of ITS batch, which the host has to wait
        for (dynenv_arrange_plan synchronises).  fixed=True or fixed=dict(max_count=M, rows=[...]): the fixed-shape mode
        (dynenv_arrange_fixed_*): inputs[i] always has rows[i] rows per (time, player) - rows past the count are zero - and the
        padded tensor always M slots; True means rows = the types' capacities and M = their sum.  Nothing is copied to the host
        and nothing waited for, so the calls can be captured into a graph.  Objects beyond rows[i] or M are dropped, earlier types
        winning, and counted per type in the persistent int32 tensor `self.dropped` (added to by every call; nothing here reads or
        zeroes it).
        padded_dtype=None: `padded` is float32.  torch.bfloat16 / torch.float16, in either mode: `padded` is written in that type; the
        embedding width must then be a multiple of 8.  (_rearrange_outputs_as: every case but the default mode's float32, which is _pad.)"""
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
        self._counts = self._obj_counts = self._base = None   # the latest rearrange_inputs call's plan (each call allocates its own)
        self.last_backward = None                             # "fused" | "rows": the route the latest backward took
        n = int(self._lib.dynenv_arrange_scratch_ints(self.E, self.nTime, self.A, self.nObjectTypes))
        self._scratch = torch.empty((n + 2,), dtype=torch.int32, device=self.device)
        self.feats = [int(t.feat) for t in types]
        if padded_dtype not in (None, torch.bfloat16, torch.float16):
            raise ValueError("padded_dtype is None (float32), torch.bfloat16 or torch.float16, got %r" % (padded_dtype,))
        self.padded_dtype = padded_dtype
        self.fixed = fixed is not None and fixed is not False
        if self.fixed:
            caps = [int(t.cap) for t in types]
            rows, max_count = (caps, sum(caps)) if fixed is True else (list(fixed["rows"]), fixed["max_count"])
            self.rows, self.max_count = [int(r) for r in rows], int(max_count)
            if len(self.rows) != self.nObjectTypes or any(not 0 <= r <= c for r, c in zip(self.rows, caps)) or self.max_count < 0:
                raise ValueError("fixed: rows[i] in 0..cap_i for each of the %d object types (caps %s) and max_count >= 0, got %r"
                                 % (self.nObjectTypes, caps, fixed))
            self._rows_c = (C.c_int32 * self.nObjectTypes)(*self.rows)
            self.dropped = torch.zeros((self.nObjectTypes,), dtype=torch.int32, device=self.device)

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def rearrange_inputs(self, obs, count_env=None):
        """obs: dense float32 device tensor [E, T, A, D]; count_env: int32 [E, 2] from BatchedDynEnv.counts() when a type
        counts per environment.  Returns (inputs, countArr) like models.py:219-250: inputs[i] float32 [N_i, feat_i] in (time, player,
        object) order; countArr = (counts int32 [type, T, P], maxCount, objCounts [T, P], slots, mask) with `countArr.base` (see
        ArrangePlan).  Every call's plan lives in buffers of its own: a countArr stays valid - for rearrange_outputs and for the
        backward of what it returned - after any number of later calls (a trainer runs backward once at the end of a rollout).
        In the fixed-shape mode: _rearrange_inputs_fixed."""
        torch = self._torch
        assert obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous()
        assert tuple(obs.shape) == (self.E, self.nTime, self.A, self.D), (tuple(obs.shape), (self.E, self.nTime, self.A, self.D))
        i32 = dict(dtype=torch.int32, device=self.device)
        counts = torch.empty((self.nObjectTypes, self.nTime, self.nPlayers), **i32)
        obj_counts = torch.empty((self.nTime, self.nPlayers), **i32)
        if self.fixed:
            return self._rearrange_inputs_fixed(obs, count_env, counts, obj_counts)
        base = torch.empty((self.nObjectTypes, self.nTime, self.nPlayers), **i32)
        self._counts, self._obj_counts, self._base = counts, obj_counts, base   # (the latest plan)
        plan = _capi.ArrPlan()
        _capi.check(self._lib.dynenv_arrange_plan(_capi.ptr(obs), self.E, self.nTime, self.A, self.D, self.types,
                                                  self.nObjectTypes, _capi.ptr(count_env), _capi.ptr(counts),
                                                  _capi.ptr(obj_counts), _capi.ptr(base), _capi.ptr(self._scratch),
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
                                                    self.nObjectTypes, _capi.ptr(counts), _capi.ptr(base), max_count,
                                                    in_ptrs, sl_ptrs, _capi.ptr(mask) if max_count else vp(0), self._stream()),
                    "dynenv_arrange_gather")
        return inputs, ArrangePlan(counts, max_count, obj_counts, slots, mask, base)

    def _rearrange_inputs_fixed(self, obs, count_env, counts, obj_counts):
        """rearrange_inputs of the fixed-shape mode: inputs[i] float32 [T*P*rows[i], feat_i] - rows[i] rows per (time, player), those past
        the kept count zero - and a countArr of the same five entries: maxCount is the Python int M, `slots` holds None per type
        (a row's slot is arithmetic here) and `.base` is None.  Two launches; nothing is read back."""
        torch = self._torch
        TP = self.nTime * self.nPlayers
        inputs = [torch.empty((TP * r, f), dtype=torch.float32, device=self.device) for r, f in zip(self.rows, self.feats)]
        mask = torch.empty((self.nTime, self.nPlayers, self.max_count), dtype=torch.uint8, device=self.device)
        vp = C.c_void_p
        in_ptrs = (vp * self.nObjectTypes)(*[t.data_ptr() if t.numel() else None for t in inputs])
        _capi.check(self._lib.dynenv_arrange_fixed_gather(_capi.ptr(obs), self.E, self.nTime, self.A, self.D, self.types,
                                                          self.nObjectTypes, _capi.ptr(count_env), self._rows_c, self.max_count,
                                                          _capi.ptr(counts), _capi.ptr(obj_counts), in_ptrs,
                                                          _capi.ptr(mask) if self.max_count else vp(0), _capi.ptr(self.dropped),
                                                          self._stream()), "dynenv_arrange_fixed_gather")
        return inputs, ArrangePlan(counts, self.max_count, obj_counts, [None] * self.nObjectTypes, mask, None)

    def _rearrange_outputs_fixed(self, outs, countArr):
        """rearrange_outputs of the fixed-shape mode: outs[i] float32 [T*P*rows[i], F] (None exactly where rows[i] == 0)"""
        torch = self._torch
        counts, max_count, _, _, mask = countArr
        if len(outs) != self.nObjectTypes:
            raise ValueError("rearrange_outputs: %d outputs for %d object types" % (len(outs), self.nObjectTypes))
        if int(max_count) != self.max_count or tuple(counts.shape) != (self.nObjectTypes, self.nTime, self.nPlayers):
            raise ValueError("rearrange_outputs: the countArr is not one of this fixed-shape arranger's")
        TP = self.nTime * self.nPlayers
        F = next((int(o.shape[1]) for o in outs if o is not None), None)
        if F is None:
            raise ValueError("rearrange_outputs: every output is None (fixed-shape mode with rows all zero)")
        for i, o in enumerate(outs):
            if o is None and self.rows[i]:
                raise ValueError("rearrange_outputs: outs[%d] is None but object type %d has rows[%d] = %d" % (i, i, i, self.rows[i]))
            if o is not None and tuple(o.shape) != (TP * self.rows[i], F):
                raise ValueError("rearrange_outputs: outs[%d] is %s, not %s" % (i, tuple(o.shape), (TP * self.rows[i], F)))
        return self._rearrange_outputs_as(outs, counts, None, self.max_count, F), [mask[t].bool() for t in range(self.nTime)]

    def _type_ptrs(self, tensors):
        return (C.c_void_p * self.nObjectTypes)(*[t.data_ptr() if (t is not None and t.numel()) else None for t in tensors])

    def _plan_of(self, countArr):
        """(counts, base, max_count, slots) of a countArr.  A plain tuple (rebuilt by the caller, no `.base`) gets its bases from
        its own counts - the exclusive prefix in (time, player) order - never from whichever call came last."""
        torch = self._torch
        counts, max_count, _, slots, _ = countArr
        base = getattr(countArr, "base", None)
        if base is None:
            flat = counts.reshape(self.nObjectTypes, -1)
            base = (torch.cumsum(flat, 1) - flat).to(torch.int32).reshape(counts.shape).contiguous()
        return counts, base, int(max_count), slots

    def rearrange_outputs(self, outs, countArr, device=None):
        """outs[i]: float32 [N_i, F] embeddings of inputs[i] (or None).  Returns (padded [T, maxCount, P, F],
        masks = list over time of bool [P, maxCount]) like models.py:252-274, and differentiable like it: when an outs[i]
        requires grad, `padded` carries a grad_fn whose backward (K5' of csrc/arranger_cols_kernels.hip, K4') hands every embedding
        row the upstream gradient's row at its slot.  The masks are not differentiable outputs."""
        torch = self._torch
        if self.fixed:
            return self._rearrange_outputs_fixed(outs, countArr)
        mask = countArr[4]
        plan = self._plan_of(countArr)
        slots = plan[3]
        if len(outs) != self.nObjectTypes:
            raise ValueError("rearrange_outputs: %d outputs for %d object types" % (len(outs), self.nObjectTypes))
        # a type without any object has out = None in the reference (:262); its counts are all zero, so it shifts nothing.
        # None for a type WITH objects would make the reference pack the later types to the left (:259-266) where the kernels
        # leave a gap of zeros: refused.
        for i, o in enumerate(outs):
            if o is None and int(slots[i].shape[0]):
                raise ValueError("rearrange_outputs: outs[%d] is None but object type %d has %d objects"
                                 % (i, i, int(slots[i].shape[0])))
        if self.padded_dtype is not None:
            F = next((int(o.shape[1]) for o in outs if o is not None), None)
            if F is None:
                raise ValueError("rearrange_outputs: every output is None")
            for i, o in enumerate(outs):   # (the kernel takes the rows' starts from the plan: the row counts are the plan's)
                if o is not None and tuple(o.shape) != (int(slots[i].shape[0]), F):
                    raise ValueError("rearrange_outputs: outs[%d] is %s, not %s" % (i, tuple(o.shape), (int(slots[i].shape[0]), F)))
            return self._rearrange_outputs_as(outs, *plan[:3], F), [mask[t].bool() for t in range(self.nTime)]
        if torch.is_grad_enabled() and any(o is not None and o.requires_grad for o in outs):
            # float32 inside the Function; another dtype is cast out here, where torch differentiates the cast
            outs = [o if o is None or o.dtype == torch.float32 else o.float() for o in outs]
            padded = _arrange_function().apply(self, plan, *outs)
        else:  # nothing to differentiate: the same launches as ever, no grad_fn
            padded = self._pad(outs, *plan)
        masks = [mask[t].bool() for t in range(self.nTime)]
        return padded, masks

    def _pad(self, outs, counts, base, max_count, slots):
        """the forward of rearrange_outputs: one pass over the padded tensor, or zero fill + one scatter per type"""
        torch = self._torch
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
            _capi.check(self._lib.dynenv_arrange_pad(ptrs, _capi.ptr(counts), _capi.ptr(base), self.nObjectTypes,
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
        return padded

    # ---- padded_dtype = bfloat16 / float16 in both modes, and float32 (None) in the fixed one: `base` is the plan's in the default
    # mode and None in the fixed one ----
    _DTYPE_CODES = {"torch.float32": _capi.ARR_F32, "torch.bfloat16": _capi.ARR_BF16, "torch.float16": _capi.ARR_F16}

    def _rearrange_outputs_as(self, outs, counts, base, max_count, F):
        """rearrange_outputs through dynenv_arrange_*_as (shapes already checked): a 16-bit padded tensor, or the fixed mode's float32 one.
        Embeddings that are all float32 are converted by the kernel; embeddings that are all of the padded tensor's dtype are copied bit
        for bit; anything else is cast to float32 out here, where torch differentiates the cast.  One launch in either mode - the default
        mode has no scatter route here and DYNENV_ARR_DENSE_MIN is not consulted.  Differentiable: every embedding gets a gradient of
        its own dtype."""
        torch = self._torch
        if not all(o is None or o.dtype == (self.padded_dtype or torch.float32) for o in outs):
            outs = [o if o is None or o.dtype == torch.float32 else o.float() for o in outs]
        outs = [o if o is None else o.contiguous() for o in outs]
        unit = 4 if self.padded_dtype is None else 8   # elements of a 16-byte unit of the padded tensor
        if F % unit or any(o is not None and o.numel() and o.data_ptr() % 16 for o in outs):
            if self.padded_dtype is None:
                raise _capi.DynEnvError("the fixed-shape arranger needs an embedding width that is a multiple of 4 (got %d) and 16-byte aligned "
                                        "embeddings; it has no per-type scatter fallback: use the default mode (fixed=None)" % F)
            raise _capi.DynEnvError("a %s padded tensor needs an embedding width that is a multiple of 8 (got %d) and 16-byte aligned embeddings: "
                                    "a 16-byte unit of it is 8 elements, and there is no per-row fallback; use padded_dtype=None"
                                    % (self.padded_dtype, F))
        if torch.is_grad_enabled() and any(o is not None and o.requires_grad for o in outs):
            return _arrange_as_function().apply(self, (counts, base, max_count), *outs)
        return self._pad_as(outs, counts, base, max_count, F)

    def _pad_as(self, outs, counts, base, max_count, F):
        """one launch: every element of the padded tensor [T, max_count, P, F] of padded_dtype (None: float32) is written"""
        padded_dtype = self.padded_dtype or self._torch.float32
        padded = self._torch.empty((self.nTime, max_count, self.nPlayers, F), dtype=padded_dtype, device=self.device)
        if max_count == 0:   # (an empty tensor has no address to hand over, and the call would launch nothing)
            return padded
        emb_code = self._DTYPE_CODES[str(next(o.dtype for o in outs if o is not None))]
        code = self._DTYPE_CODES[str(padded_dtype)]
        if base is None:
            _capi.check(self._lib.dynenv_arrange_fixed_pad_as(self._type_ptrs(outs), emb_code, _capi.ptr(counts), self._rows_c, self.nObjectTypes,
                                                              self.nTime, self.nPlayers, max_count, F, _capi.ptr(padded), code, self._stream()),
                        "dynenv_arrange_fixed_pad_as")
        else:
            _capi.check(self._lib.dynenv_arrange_pad_as(self._type_ptrs(outs), emb_code, _capi.ptr(counts), _capi.ptr(base), self.nObjectTypes,
                                                        self.nTime, self.nPlayers, max_count, F, _capi.ptr(padded), code, self._stream()),
                        "dynenv_arrange_pad_as")
        return padded

    def _unpad_as(self, grad, rows, emb_dtype, F, wanted, counts, base, max_count):
        """the backward of _pad_as, one launch: grad [T, max_count, P, F] -> per type [rows[i], F] of the embeddings' dtype - widened exactly
        to float32 or copied bit for bit - None where rows[i] is None or the gradient is not wanted.  Every row is written: the fixed
        mode's rows behind the kept ones are zero."""
        torch = self._torch
        padded_dtype = self.padded_dtype or torch.float32
        g = grad.contiguous()   # (an attention layer often hands back a permuted view)
        if g.dtype != padded_dtype:
            g = g.to(padded_dtype)
        if g.data_ptr() % 16:
            g = g.clone()
        assert tuple(g.shape) == (self.nTime, max_count, self.nPlayers, F), tuple(g.shape)
        make = torch.zeros if max_count == 0 else torch.empty   # (M == 0: nothing is launched and every gradient row is zero)
        grads = [make((n, F), dtype=emb_dtype, device=g.device) if (n is not None and w) else None for n, w in zip(rows, wanted)]
        if base is not None:
            self.last_backward = None
        if max_count == 0 or not any(ge is not None and ge.shape[0] for ge in grads):
            return grads
        emb_code, code = self._DTYPE_CODES[str(emb_dtype)], self._DTYPE_CODES[str(padded_dtype)]
        if base is None:
            _capi.check(self._lib.dynenv_arrange_fixed_pad_backward_as(_capi.ptr(g), code, _capi.ptr(counts), self._rows_c, self.nObjectTypes,
                                                                       self.nTime, self.nPlayers, max_count, F, self._type_ptrs(grads),
                                                                       emb_code, self._stream()), "dynenv_arrange_fixed_pad_backward_as")
        else:
            _capi.check(self._lib.dynenv_arrange_pad_backward_as(_capi.ptr(g), code, _capi.ptr(counts), _capi.ptr(base), self.nObjectTypes,
                                                                 self.nTime, self.nPlayers, max_count, F, self._type_ptrs(grads), emb_code,
                                                                 self._stream()), "dynenv_arrange_pad_backward_as")
            self.last_backward = "fused"
        return grads

    def _unpad(self, grad, rows, F, wanted, counts, base, max_count, slots):
        """the backward of _pad: grad [T, maxCount, P, F] -> per type float32 [N_i, F] (None where rows[i] is None or the gradient
        is not wanted).  One fused pass when F % 4 == 0 and every buffer is 16-byte aligned, whichever forward ran (its cost goes
        with the objects, not with the padding); else one row gather per type.  self.last_backward names the route taken."""
        torch = self._torch
        g = grad.contiguous()   # (an attention layer often hands back a permuted view)
        if g.dtype != torch.float32:
            g = g.float()
        assert tuple(g.shape) == (self.nTime, max_count, self.nPlayers, F), tuple(g.shape)
        # every row is written: no zero fill
        grads = [torch.empty((n, F), dtype=torch.float32, device=g.device) if (n is not None and w) else None
                 for n, w in zip(rows, wanted)]
        live = [ge is not None and ge.shape[0] > 0 for ge in grads]
        self.last_backward = None
        if max_count == 0 or not any(live):
            return grads
        vp = C.c_void_p
        if F % 4 == 0 and g.data_ptr() % 16 == 0 and all(ge.data_ptr() % 16 == 0 for ge, l in zip(grads, live) if l):
            ptrs = (vp * self.nObjectTypes)(*[ge.data_ptr() if l else None for ge, l in zip(grads, live)])
            _capi.check(self._lib.dynenv_arrange_pad_backward(_capi.ptr(g), _capi.ptr(counts), _capi.ptr(base), self.nObjectTypes,
                                                              self.nTime, self.nPlayers, max_count, F, ptrs, self._stream()),
                        "dynenv_arrange_pad_backward")
            self.last_backward = "fused"
        else:
            for i, ge in enumerate(grads):
                if live[i]:
                    _capi.check(self._lib.dynenv_arrange_scatter_backward(_capi.ptr(g), _capi.ptr(slots[i]), int(ge.shape[0]), F,
                                                                          _capi.ptr(ge), self._stream()),
                                "dynenv_arrange_scatter_backward")
            self.last_backward = "rows"
        return grads


class ArrangePlan(tuple):
    """The countArr of GpuInOutArranger.rearrange_inputs: the five entries (counts, maxCount, objCounts, slots, mask) - the
    reference's three (models.py:248) in its order, then the two the kernels add - and, as the attribute `.base`, the int32
    [type, T, P] start of every (time, player)'s objects inside inputs[i].  An attribute, not a sixth entry: callers unpack five."""

    def __new__(cls, counts, max_count, obj_counts, slots, mask, base):
        self = tuple.__new__(cls, (counts, max_count, obj_counts, slots, mask))
        self.base = base
        return self


# torch is imported on first use (the package itself imports without it): the autograd Function and the nn.Module are built then.
_lazy = {}


def _arrange_function():
    if "fn" not in _lazy:
        import torch
        from torch.autograd.function import once_differentiable

        class ArrangeOutputs(torch.autograd.Function):
            """padded = arranger._pad(outs, plan); d padded / d outs[i] = arranger._unpad.  The plan is the forward call's own."""

            @staticmethod
            def forward(ctx, arr, plan, *outs):
                ctx.arr, ctx.plan = arr, plan
                ctx.rows = [None if o is None else int(o.shape[0]) for o in outs]
                ctx.F = next(int(o.shape[1]) for o in outs if o is not None)
                return arr._pad(outs, *plan)

            @staticmethod
            @once_differentiable
            def backward(ctx, grad):
                grads = ctx.arr._unpad(grad, ctx.rows, ctx.F, ctx.needs_input_grad[2:], *ctx.plan)
                return (None, None) + tuple(grads)

        _lazy["fn"] = ArrangeOutputs
    return _lazy["fn"]


def _arrange_as_function():
    if "as_fn" not in _lazy:
        import torch
        from torch.autograd.function import once_differentiable

        class ArrangeOutputsAs(torch.autograd.Function):
            """padded = arranger._pad_as(outs, plan) in the arranger's padded_dtype (None: float32); d padded / d outs[i] = arranger._unpad_as, in outs[i]'s own
            dtype.  plan = (counts, base, max_count) of the forward call, base None in the fixed mode."""

            @staticmethod
            def forward(ctx, arr, plan, *outs):
                ctx.arr, ctx.plan = arr, plan
                ctx.rows = [None if o is None else int(o.shape[0]) for o in outs]
                first = next(o for o in outs if o is not None)
                ctx.F, ctx.emb_dtype = int(first.shape[1]), first.dtype
                return arr._pad_as(outs, *plan, ctx.F)

            @staticmethod
            @once_differentiable
            def backward(ctx, grad):
                return (None, None) + tuple(ctx.arr._unpad_as(grad, ctx.rows, ctx.emb_dtype, ctx.F, ctx.needs_input_grad[2:], *ctx.plan))

        _lazy["as_fn"] = ArrangeOutputsAs
    return _lazy["as_fn"]


def _input_layer_class():
    if "layer" not in _lazy:
        import torch

        class GpuInputLayer(torch.nn.Module):
            """The reference's InputLayer (models.py:278-307) over the dense observation tensor: rearrange_inputs -> one embedding
            block per object type -> rearrange_outputs, differentiable down to the blocks' parameters.

            GpuInputLayer(blocks, types, nEnvs, nAgents, nTime, obs_dim): `blocks` is the caller's own nn.ModuleList, one module per
            object type of `types` (groups_for(env)[...]), each mapping [N, feat_i] -> [N, F]; the embedding network is the trainer's.
            forward(obs, count_env=None) -> (padded [T, maxCount, E*A, F], masks).  A type without objects in this call does not run
            its block and contributes None, as EmbedBlock returns for an empty input (:112-116): its parameters get no gradient.

            fixed=True / fixed=dict(max_count=M, rows=[...]) (GpuInOutArranger): the fixed-shape mode - padded is [T, M, E*A, F] whatever
            the batch holds, no call waits for the device, and the whole forward can be captured into a graph.  Every block then runs on
            every call, on rows[i] rows per (time, player), because x.shape[0] is no longer decided by the batch; only a type with
            rows[i] == 0 contributes None.  CAVEAT: the blocks also see the all-zero rows behind each player's objects (their output is
            discarded and their gradient is zero), so they must be ROW-WISE - Linear, LayerNorm, activations, as the reference's
            EmbedBlock; a block that mixes rows (BatchNorm in training mode, attention across rows) would let the zero rows leak into
            the real ones.

            padded_dtype=torch.bfloat16 / torch.float16 (GpuInOutArranger), in either mode: `padded` comes out in that type - what a
            network under torch.autocast reads - from float32 blocks (an EmbedBlock ends in a LayerNorm: float32 under autocast) or from
            blocks that already return it; the blocks' parameters get the gradients they would get through a float32 padded tensor cast
            to that type."""

            def __init__(self, blocks, types, nEnvs, nAgents, nTime, obs_dim, fixed=None, padded_dtype=None):
                super().__init__()
                if len(blocks) != len(types):
                    raise ValueError("GpuInputLayer: %d blocks for %d object types" % (len(blocks), len(types)))
                self.blocks = blocks if isinstance(blocks, torch.nn.ModuleList) else torch.nn.ModuleList(blocks)
                self.arranger = GpuInOutArranger(types, nEnvs, nAgents, nTime, obs_dim, fixed=fixed, padded_dtype=padded_dtype)

            def forward(self, obs, count_env=None):
                inputs, countArr = self.arranger.rearrange_inputs(obs, count_env)
                outs = [block(x) if x.shape[0] else None for block, x in zip(self.blocks, inputs)]
                return self.arranger.rearrange_outputs(outs, countArr)

        GpuInputLayer.__qualname__ = "GpuInputLayer"
        _lazy["layer"] = GpuInputLayer
    return _lazy["layer"]


def _embed_classes():
    if "embed" not in _lazy:
        import torch
        nn = torch.nn

        class EmbedBlock(nn.Module):
            """The reference's embedding block for one object type (models.py:99-124), parameter for parameter and name for name:
            Linear(feat -> F/2, no bias), LeakyReLU(0.1), LayerNorm(F/2), Linear(F/2 -> F, no bias), LeakyReLU(0.1), LayerNorm(F)."""

            def __init__(self, inputs, features, device=None):
                super().__init__()
                self.Layer1 = nn.Linear(inputs, features // 2, bias=False, device=device)
                self.relu = nn.LeakyReLU(0.1)
                self.bn1 = nn.LayerNorm(features // 2, device=device)
                self.Layer2 = nn.Linear(features // 2, features, bias=False, device=device)
                self.bn2 = nn.LayerNorm(features, device=device)

            def forward(self, x):
                x = self.bn1(self.relu(self.Layer1(x)))
                return self.bn2(self.relu(self.Layer2(x)))

        class GpuEmbedInputLayer(nn.Module):
            """The reference's WHOLE InputLayer (models.py:278-307) over the dense observation tensor, embedding blocks included:
            GpuEmbedInputLayer(types, features, nEnvs, nAgents, nTime, obs_dim, fixed=None, padded_dtype=None) owns `blocks`, one EmbedBlock
            (models.py:99-124) per object type of `types` (groups_for(env)[...]), created on the arranger's device under the reference's
            parameter names (Layer1.weight, bn1.weight, bn1.bias, Layer2.weight, bn2.weight, bn2.bias): an InputLayer.state_dict() of
            the reference loads with strict=True.  forward(obs, count_env=None) -> (padded [T, maxCount, E*A, F], masks) with the shapes,
            masks, `arranger.dropped` accounting and `padded_dtype` meaning of GpuInputLayer (fixed=, padded_dtype=: GpuInOutArranger).

            Two routes; `last_route` names the one the latest forward took.
              "blocks"  when gradients are enabled and a parameter requires one: GpuInputLayer's route - rearrange_inputs, the blocks
                        as torch modules, rearrange_outputs - unchanged and differentiable.
              "fused"   otherwise (acting in a rollout, evaluation, look-ahead, the no_grad value bootstrap): one kernel reads the
                        observation rows and writes the padded tensor (dynenv_arrange_embed_pad, csrc/arranger_embed_kernels.hip);
                        neither inputs[i], nor an activation, nor the embeddings exist.  Fixed mode: dynenv_arrange_fixed_gather without
                        inputs (counts, mask, dropped), then the kernel - nothing is waited for, so the route is capturable.  Default
                        mode: dynenv_arrange_plan (its one synchronisation, as ever), the gather for the mask alone, then the kernel.
              "blocks (fallback: ...)"  where no gradient is wanted but the kernel does not take the module: F other than 64 or 128, a
                        type of more than 16 features, parameters that are not float32, contiguous and on the arranger's device, a
                        LayerNorm without affine parameters - or DYNENV_ARR_EMBED_FUSED=0 in the environment.  Nothing is raised.
            AUTOCAST.  The fused route computes in float32 whatever torch.autocast says - only the store converts, to `padded_dtype` -
            while the unfused route's Linears run in 16 bits under autocast (its LayerNorms stay float32): under autocast the two
            routes differ by the 16-bit rounding of the two products, the fused one being the more exact."""

            def __init__(self, types, features, nEnvs, nAgents, nTime, obs_dim, fixed=None, padded_dtype=None):
                super().__init__()
                self.arranger = GpuInOutArranger(types, nEnvs, nAgents, nTime, obs_dim, fixed=fixed, padded_dtype=padded_dtype)
                self.features = int(features)
                self.blocks = nn.ModuleList([EmbedBlock(int(t.feat), self.features, device=self.arranger.device) for t in types])
                self.last_route = None

            def _not_fusable(self):
                """why the kernel does not take this module as it stands, or None"""
                arr = self.arranger
                if os.environ.get("DYNENV_ARR_EMBED_FUSED", "1") == "0":
                    return "DYNENV_ARR_EMBED_FUSED=0"
                if self.features not in (64, 128):
                    return "F = %d, not 64 or 128" % self.features
                if max(arr.feats) > 16:
                    return "an object type of more than 16 features"
                b0 = self.blocks[0]
                for b in self.blocks:
                    if (b.bn1.eps, b.bn2.eps, b.relu.negative_slope) != (b0.bn2.eps, b0.bn2.eps, b0.relu.negative_slope):
                        return "blocks that differ in eps or slope"
                    if not (b.bn1.elementwise_affine and b.bn2.elementwise_affine and b.bn1.bias is not None and b.bn2.bias is not None):
                        return "a LayerNorm without affine parameters"
                    for p in b.parameters():
                        if p.dtype != torch.float32 or not p.is_contiguous() or p.device != arr.device:
                            return "parameters that are not float32, contiguous and on %s" % (arr.device,)
                return None

            def forward(self, obs, count_env=None):
                if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
                    self.last_route = "blocks"
                    return self._forward_blocks(obs, count_env)
                why = self._not_fusable()
                if why is not None:
                    self.last_route = "blocks (fallback: %s)" % why
                    return self._forward_blocks(obs, count_env)
                self.last_route = "fused"
                return self._forward_fused(obs, count_env)

            def _forward_blocks(self, obs, count_env):
                inputs, countArr = self.arranger.rearrange_inputs(obs, count_env)
                outs = [block(x) if x.shape[0] else None for block, x in zip(self.blocks, inputs)]
                return self.arranger.rearrange_outputs(outs, countArr)

            def _forward_fused(self, obs, count_env):
                arr = self.arranger
                lib, vp, n = arr._lib, C.c_void_p, arr.nObjectTypes
                assert obs.is_cuda and obs.dtype == torch.float32 and obs.is_contiguous()
                assert tuple(obs.shape) == (arr.E, arr.nTime, arr.A, arr.D), (tuple(obs.shape), (arr.E, arr.nTime, arr.A, arr.D))
                i32 = dict(dtype=torch.int32, device=arr.device)
                counts = torch.empty((n, arr.nTime, arr.nPlayers), **i32)
                obj_counts = torch.empty((arr.nTime, arr.nPlayers), **i32)
                if arr.fixed:
                    max_count = arr.max_count
                    mask = torch.empty((arr.nTime, arr.nPlayers, max_count), dtype=torch.uint8, device=arr.device)
                    _capi.check(lib.dynenv_arrange_fixed_gather(_capi.ptr(obs), arr.E, arr.nTime, arr.A, arr.D, arr.types, n, _capi.ptr(count_env),
                                                                arr._rows_c, max_count, _capi.ptr(counts), _capi.ptr(obj_counts), None,
                                                                _capi.ptr(mask) if max_count else vp(0), _capi.ptr(arr.dropped), arr._stream()),
                                "dynenv_arrange_fixed_gather")
                else:
                    base = torch.empty((n, arr.nTime, arr.nPlayers), **i32)
                    plan = _capi.ArrPlan()
                    _capi.check(lib.dynenv_arrange_plan(_capi.ptr(obs), arr.E, arr.nTime, arr.A, arr.D, arr.types, n, _capi.ptr(count_env),
                                                        _capi.ptr(counts), _capi.ptr(obj_counts), _capi.ptr(base), _capi.ptr(arr._scratch),
                                                        C.byref(plan), arr._stream()), "dynenv_arrange_plan")
                    max_count = int(plan.max_count)
                    mask = torch.empty((arr.nTime, arr.nPlayers, max_count), dtype=torch.uint8, device=arr.device)
                    if max_count:   # (the gather for the mask alone: no inputs, no slots)
                        _capi.check(lib.dynenv_arrange_gather(_capi.ptr(obs), arr.E, arr.nTime, arr.A, arr.D, arr.types, n, _capi.ptr(counts),
                                                              _capi.ptr(base), max_count, None, None, _capi.ptr(mask), arr._stream()),
                                    "dynenv_arrange_gather")
                padded_dtype = arr.padded_dtype or torch.float32
                padded = torch.empty((arr.nTime, max_count, arr.nPlayers, self.features), dtype=padded_dtype, device=arr.device)
                if max_count:
                    blocks = (_capi.EmbedBlock * n)(*[_capi.EmbedBlock(*[p.data_ptr() for p in (b.Layer1.weight, b.bn1.weight, b.bn1.bias,
                                                                                               b.Layer2.weight, b.bn2.weight, b.bn2.bias)])
                                                      for b in self.blocks])
                    b0 = self.blocks[0]
                    _capi.check(lib.dynenv_arrange_embed_pad(_capi.ptr(obs), arr.E, arr.nTime, arr.A, arr.D, arr.types, n, _capi.ptr(counts), max_count,
                                                             blocks, self.features, float(b0.relu.negative_slope), float(b0.bn2.eps),
                                                             _capi.ptr(padded), arr._DTYPE_CODES[str(padded_dtype)], arr._stream()),
                                "dynenv_arrange_embed_pad")
                self.last_counts, self.last_obj_counts = counts, obj_counts   # (the latest fused call's plan, for whoever wants the counts)
                return padded, [mask[t].bool() for t in range(arr.nTime)]

        EmbedBlock.__qualname__, GpuEmbedInputLayer.__qualname__ = "EmbedBlock", "GpuEmbedInputLayer"
        _lazy["embed"] = (EmbedBlock, GpuEmbedInputLayer)
    return _lazy["embed"]


def __getattr__(name):
    if name == "GpuInputLayer":
        return _input_layer_class()
    if name in ("EmbedBlock", "GpuEmbedInputLayer"):
        return _embed_classes()[name == "GpuEmbedInputLayer"]
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
