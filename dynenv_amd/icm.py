"""The curiosity module behind the rollout storage: the reference's ICMNet (DynEnv/models/icm.py) - forward and inverse dynamics over a
stored rollout and the two curiosity losses of ICMNet._calc_loss - differentiable through torch where a gradient is wanted and ONE call
(dynenv_icm_losses, csrc/icm_kernels.hip) where none is.  Neither route reads the host: the reference's one-hot loop (icm.py:167-179, one
.item() per action) is a scatter_ here and a gather in the kernel, its early return and boolean indexing are torch.where and sums."""
import collections
import ctypes as C
import os

from . import _capi

HIDDEN, HIDDEN_PAD = 140, 160   # DYNENV_ICM_HIDDEN, DYNENV_ICM_HIDDEN_PAD
MAX_ROWS, MAX_GROUPS, MAX_GROUP, MAX_COLS = 32, 8, 16, 8   # the kernel's limits (include/dynenv.h)
FUSED_K = (64, 128, 256)
FUSED_BACKWARD_K = (64, 128)   # what dynenv_icm_backward takes: at 256 the weight gradients do not fit the register file

ICMLosses = collections.namedtuple("ICMLosses", ["loss", "inverse", "forward", "long_horizon_forward"])


class _Discrete(object):
    """what ActorBlock looks at of a MultiDiscrete space"""

    def __init__(self, nvec):
        self.nvec = [int(n) for n in nvec]


def _blocks(groups):
    """groups -> the list of the action descriptor's members as lists of group sizes: a flat sequence of ints is ONE MultiDiscrete
    member (policy.nvec of Driving and RoboCup); a space with .spaces, or a sequence of spaces, keeps its members"""
    members = groups.spaces if hasattr(groups, "spaces") else list(groups)
    if all(hasattr(m, "nvec") for m in members) and members:
        return [[int(n) for n in m.nvec] for m in members]
    assert members and not any(hasattr(m, "shape") or hasattr(m, "low") for m in members), \
        "GpuICM supports all-discrete action spaces only: a cross-entropy has no meaning for a Box block"
    return [[int(n) for n in members]]


# torch is imported on first use (the package itself imports without it): the nn.Modules are built then.
_lazy = {}


def _classes():
    if "icm" not in _lazy:
        import torch
        from .policy import _classes as policy_classes
        nn = torch.nn
        ActorLayer = policy_classes()["ActorLayer"]

        class ForwardNet(nn.Module):
            """icm.py:112-146"""

            def __init__(self, feat_size, action_size, device=None):
                super().__init__()
                self.fc1 = nn.Linear(feat_size + action_size, HIDDEN, device=device)
                self.fc2 = nn.Linear(HIDDEN, feat_size, device=device)
                self.relu = nn.LeakyReLU(0.1)

            def forward(self, x):
                return self.fc2(self.relu(self.fc1(x)))

        class AttentionNet(nn.Module):
            """icm.py:243-253"""

            def __init__(self, attention_size, device=None):
                super().__init__()
                self.attention = nn.Linear(attention_size, attention_size, device=device)

            def forward(self, target, attn=None):
                return target * torch.softmax(self.attention(target if attn is None else attn), dim=-1)

        class ICMDynamics(nn.Module):
            """icm.py:182-240 without AttentionTarget.ICM: the forward net and the inverse net"""

            def __init__(self, feat_size, blocks, device=None):
                super().__init__()
                self.fwd_net = ForwardNet(feat_size, sum(sum(b) for b in blocks), device=device)
                self.inv_net = ActorLayer(feat_size * 2, [_Discrete(b) for b in blocks], device=device)

        class LongHorizonCuriosityLoss(nn.Module):
            """icm.py:256-298"""

            def __init__(self, attention_size, device=None):
                super().__init__()
                self.attention = AttentionNet(attention_size, device=device)

            def forward(self, pred_states, true_states):
                mse_loss, weight = 0.0, 1.0
                for pred, true in zip(pred_states, true_states):
                    step = (pred - true) ** 2
                    mse_loss = mse_loss + (weight * step).mean()
                    weight = self.attention(step)
                return mse_loss

        class LongHorizonForwardNet(nn.Module):
            """icm.py:301-335"""

            def __init__(self, feat_size, action_size, num_pred_steps, device=None):
                super().__init__()
                self.fwd_nets = nn.ModuleList([ForwardNet(feat_size, action_size, device=device) for _ in range(num_pred_steps)])

            def forward(self, current_feature, one_hot_actions):
                preds = [current_feature]
                for net, one_hot in zip(self.fwd_nets, one_hot_actions):
                    preds.append(net(torch.cat((preds[-1], one_hot), 1)))
                return preds[1:]

        class GpuICM(nn.Module):
            """The reference's ICMNet (icm.py:13-109) parameter for parameter and name for name - pred_net.fwd_net.fc1/fc2,
            pred_net.inv_net.blocks.*.Layer.*, loss_long_horizon_curiosity.attention.attention, long_horizon_fwd_net.fwd_nets.<t>.fc1/fc2
            and, with loss_attention, loss_attn.attention - so that an ICMNet.state_dict() loads with strict=True.

            feature_size is K, the storage's feature width (the reference's feat_size * 2: 128 with its main.py); groups is policy.nvec,
            the sizes of the discrete action groups (a flat sequence: one MultiDiscrete member; an action space or a sequence of spaces
            keeps its members as the reference's action_descriptor does), G = len(groups), N = sum(groups); rollout_size the number of
            the long-horizon nets.  ONLY ALL-DISCRETE ACTION SPACES are supported: the reference's F.cross_entropy on zip(action_preds,
            actions) has no meaning for a Box block.  loss_attention=True is the reference's RCM configuration (AttentionTarget.ICM_LOSS
            with SINGLE_ATTENTION); AttentionTarget.ICM is not offered (the reference's fwd_att is sized feat + len(descriptor) and does
            not fit its own one-hot input).

            forward(features [T + 1, P, K], actions [T, AD, P], agent_finished bool [T, P] or None, long_horizon=False) ->
            ICMLosses(loss, inverse, forward, long_horizon_forward), device tensors of no dimension - the storage's buffers as they are.
            It is ICMNet.forward + _calc_loss as they run, with mask = ~agent_finished and n its number of true entries, counted on
            the device:
                forward = forward_coeff * sum_mask sum_k (pred - next)^2 / (n K)      (F.mse_loss over the gathered rows)
                inverse = icm_beta * mean_g(sum_mask CE_g / n),  CE_g = logsumexp(l_g) - l_g[a_g]
                loss    = inverse + forward
            both exactly 0 where n == 0 (torch.where on the device: the reference's early return).  Only the action columns 0..G-1 are
            read.  An action value is rounded to an integer and clamped into 0..n_g-1 for addressing; a value that had to be clamped
            sets bit 0 of `status`, an int32 [1] on the device that nothing here clears (the reference raises an IndexError there).

            rows(features, actions) -> (curiosity [T, P], inverse_ce [T, G, P]), float32, without a gradient: the per-agent forward
            error mean_k (pred - next)^2 - the intrinsic-reward signal of the ICM paper - and the cross-entropy per group in log_probs'
            layout.  Finished agents are included: the mask belongs to the losses.

            Routes; `last_route` names the one the latest forward or rows took.
              "torch"  when gradients are enabled and an input or a parameter requires one: the reference's statements - the one-hot by
                       scatter_, cat, the Linears - then the masked sums above.  Differentiable through the parameters and through
                       `features` (the reference's storage does not detach them: the extractor trains through ICM).  No host read.
              "fused"  where no gradient is wanted: one call of dynenv_icm_losses.  K of 64, 128 or 256, G <= 8 groups of at most 16,
                       N <= 32, AD <= 8, float32 contiguous inputs on the device.  A packed copy of the weights in w_dtype is kept and
                       refreshed IN PLACE (fixed pointers, torch ops on the stream) when a parameter's version changes.
              "torch (fallback: why)"  where no gradient is wanted but the kernel does not take the call - loss_attention=True and
                       DYNENV_ICM_FUSED=0 in the environment among the reasons.  Nothing is raised.
              "fused (backward)"  only with fused_backward=True, when gradients are enabled and an input or a parameter requires
                       one: the losses are the "fused" route's, bit for bit, behind a torch.autograd.Function, and loss.backward()
                       is ONE call of dynenv_icm_backward (csrc/icm_backward_kernels.hip), which recomputes the forward per row from
                       the saved inputs - nothing else is saved - and fills the .grad of exactly pred_net.* and, where wanted, of
                       `features`.  The "fused" route's conditions, K of 64 or 128; otherwise "torch (fallback: why)", differentiable
                       as the torch route is.  Gradient and workspace buffers are the module's, at fixed addresses; the transposed
                       packed copies the kernel reads are refreshed with the others.  Not twice differentiable.
            The routes differ by the rounding of the matrix products' operands to w_dtype.

            Deliberate differences from the reference.
              * long_horizon_forward is not part of `loss` there either (ICMLosses.prepare_losses, loss_descriptors.py:49-50), so the
                long-horizon nets never receive a gradient.  Here their parameters exist so that a checkpoint loads; the term is
                evaluated through torch, detached, only with long_horizon=True (long_horizon_coeff * the reference's value, 0 where
                n == 0), and is a zero tensor otherwise.
              * The fields are device tensors: nothing is copied to the host (the reference's prepare_losses calls .item()).
              * A clamped action raises nothing: it sets the status bit."""

            def __init__(self, feature_size, groups, rollout_size, forward_coeff=1e-2, icm_beta=1e-2, long_horizon_coeff=0.0, loss_attention=False,
                         w_dtype=torch.bfloat16, device=None, fused_backward=False):
                super().__init__()
                self.feature_size, self.rollout_size = int(feature_size), int(rollout_size)
                blocks = _blocks(groups)
                self.groups = [n for b in blocks for n in b]
                assert self.groups and min(self.groups) >= 1, "an action space has a discrete group"
                self.forward_coeff, self.icm_beta, self.long_horizon_coeff = float(forward_coeff), float(icm_beta), float(long_horizon_coeff)
                self.w_dtype = w_dtype
                assert self.w_dtype in (torch.bfloat16, torch.float16), "w_dtype is torch.bfloat16 or torch.float16"
                K, N = self.feature_size, sum(self.groups)
                self.pred_net = ICMDynamics(K, blocks, device=device)
                self.loss_attn_flag = bool(loss_attention)
                if self.loss_attn_flag:
                    self.loss_attn = AttentionNet(K, device=device)
                self.loss_long_horizon_curiosity = LongHorizonCuriosityLoss(K, device=device)
                self.long_horizon_fwd_net = LongHorizonForwardNet(K, N, self.rollout_size, device=device)
                starts = [sum(self.groups[:g]) for g in range(len(self.groups))]
                self.register_buffer("_starts", torch.tensor(starts, dtype=torch.int64, device=device), persistent=False)
                self.register_buffer("_last", torch.tensor(self.groups, dtype=torch.int64, device=device) - 1, persistent=False)
                self.register_buffer("status", torch.zeros(1, dtype=torch.int32, device=device), persistent=False)
                self.fused_backward = bool(fused_backward)
                self._route = None
                self._packed = None
                self._bwd = None

            @property
            def last_route(self):
                return self._route

            def _linears(self):
                return [l for b in self.pred_net.inv_net.blocks for l in b.Layer]

            # ---- the torch route
            def _indices(self, actions):
                """actions [T, AD, P] -> int64 [T, G, P] inside the groups; a value that had to be clamped sets the status bit"""
                G = len(self.groups)
                with torch.no_grad():
                    v = actions[:, :G].detach().round()
                    last = self._last.to(v.dtype).view(1, G, 1)
                    ok = (v >= 0) & (v <= last)
                    idx = torch.where(ok, v, torch.where(v > last, last, torch.zeros_like(v))).long()
                    self.status.bitwise_or_((~ok).any().to(torch.int32))
                return idx

            def _one_hot(self, idx, dtype):
                T, G, P = idx.shape
                one_hot = torch.zeros((T, P, sum(self.groups)), dtype=dtype, device=idx.device)
                return one_hot.scatter_(2, (idx + self._starts.view(1, G, 1)).permute(0, 2, 1), 1.0)

            def _rows_torch(self, features, idx):
                """-> (se [T, P, K]: the squared error of the prediction, ce: a list of G tensors [T, P]), float32 or wider"""
                cur, nxt = features[:-1], features[1:]
                one_hot = self._one_hot(idx, features.dtype)
                pred = self.pred_net.fwd_net(torch.cat((cur, one_hot), 2))
                logits = self.pred_net.inv_net(torch.cat((cur, nxt), 2))
                wide = lambda x: x.float() if x.dtype in (torch.bfloat16, torch.float16) else x   # noqa: E731  (what mse_loss and cross_entropy do under autocast)
                se = (wide(pred) - nxt) ** 2
                ce = []
                for g, l in enumerate(logits):
                    l = wide(l)
                    ce.append(-torch.log_softmax(l, dim=-1).gather(2, idx[:, g].unsqueeze(-1)).squeeze(-1))   # (F.cross_entropy's own two steps)
                return se, ce, one_hot

            def _long_horizon(self, features, one_hot, some):
                with torch.no_grad():
                    preds = self.long_horizon_fwd_net(features[0], one_hot)
                    value = self.loss_long_horizon_curiosity(preds, features[1:])
                    value = torch.as_tensor(value, dtype=features.dtype, device=features.device)
                    return torch.where(some, self.long_horizon_coeff * value, torch.zeros_like(value))

            def _forward_torch(self, features, actions, agent_finished, long_horizon):
                T, P, K = features.shape[0] - 1, features.shape[1], features.shape[2]
                idx = self._indices(actions)
                se, ce, one_hot = self._rows_torch(features, idx)
                mask = torch.ones((T, P), dtype=torch.bool, device=features.device) if agent_finished is None else ~(agent_finished != 0)
                n = mask.sum()
                some = n > 0
                nf = n.clamp(min=1).to(se.dtype)
                zero = torch.zeros((), dtype=se.dtype, device=se.device)
                if self.loss_attn_flag:   # icm.py:93: not masked, as it runs
                    fwd = self.loss_attn(se, features[1:]).mean()
                else:
                    fwd = torch.where(mask.unsqueeze(-1), se, zero).sum() / (nf * K)
                inv = torch.stack([torch.where(mask, c, zero).sum() / nf for c in ce]).mean()
                fwd = torch.where(some, self.forward_coeff * fwd, zero)
                inv = torch.where(some, self.icm_beta * inv, zero)
                lh = self._long_horizon(features.detach(), one_hot, some) if long_horizon else zero.detach().clone()
                return ICMLosses(inv + fwd, inv, fwd, lh)

            # ---- the fused route
            def _not_fusable(self, features, actions, agent_finished, for_loss=True):
                """why the kernel does not take this call, or None"""
                K, G = self.feature_size, len(self.groups)
                if os.environ.get("DYNENV_ICM_FUSED", "") == "0":
                    return "DYNENV_ICM_FUSED=0"
                if for_loss and self.loss_attn_flag:
                    return "loss_attention=True"
                if K not in FUSED_K:
                    return "K = %d, not 64, 128 or 256" % K
                if G > MAX_GROUPS or max(self.groups) > MAX_GROUP or sum(self.groups) > MAX_ROWS or actions.shape[1] > MAX_COLS:
                    return "an action space beyond %d groups of %d, %d rows or %d columns" % (MAX_GROUPS, MAX_GROUP, MAX_ROWS, MAX_COLS)
                if not features.is_cuda:
                    return "features that are not on the device"
                dev = features.device
                for name, t, dtypes in (("features", features, (torch.float32,)), ("actions", actions, (torch.float32,)),
                                        ("agent_finished", agent_finished, (torch.bool, torch.uint8))):
                    if t is not None and (t.dtype not in dtypes or not t.is_contiguous() or t.device != dev or t.data_ptr() % 16):
                        return "%s that is not %s, contiguous, 16-byte aligned and on %s" % (name, " / ".join(str(d) for d in dtypes), dev)
                for p in list(self.pred_net.parameters()) + [self.status]:
                    if (p.dtype != torch.float32 and p is not self.status) or p.device != dev:
                        return "parameters that are not float32 and on %s" % (dev,)
                return None

            def _params(self):
                """the parameters of pred_net in the order the fused backward returns their gradients"""
                fwd = self.pred_net.fwd_net
                return [fwd.fc1.weight, fwd.fc1.bias, fwd.fc2.weight, fwd.fc2.bias] + [q for l in self._linears() for q in (l.weight, l.bias)]

            def _weights(self, dev, backward=False):
                """the packed operands of dynenv_icm_t, made once per device and refreshed in place when a parameter changed; with
                `backward` (and from then on) the transposed copies of dynenv_icm_bwd_t too, refreshed in the same pass"""
                K, N, dt = self.feature_size, sum(self.groups), self.w_dtype
                fwd, lin = self.pred_net.fwd_net, self._linears()
                params = [fwd.fc1.weight, fwd.fc1.bias, fwd.fc2.weight, fwd.fc2.bias] + [q for l in lin for q in (l.weight, l.bias)]
                key = tuple((p.data_ptr(), p._version) for p in params)
                pk = self._packed
                z = lambda shape, d: torch.zeros(shape, dtype=d, device=dev)   # noqa: E731
                if pk is None or pk["dev"] != dev or pk["dt"] != dt:
                    pk = dict(dev=dev, dt=dt, key=None, w1=z((HIDDEN_PAD, K), dt), w1_act=z((N, HIDDEN_PAD), torch.float32), b1=z((HIDDEN_PAD,), torch.float32),
                              w2=z((K, HIDDEN_PAD), dt), b2=z((K,), torch.float32), inv_w=z((MAX_ROWS, 2 * K), dt), inv_b=z((MAX_ROWS,), torch.float32))
                    c = _capi.Icm()
                    c.fwd_w1, c.fwd_w1_act, c.fwd_b1, c.fwd_w2, c.fwd_b2 = (pk[k].data_ptr() for k in ("w1", "w1_act", "b1", "w2", "b2"))
                    c.inv_w, c.inv_b = pk["inv_w"].data_ptr(), pk["inv_b"].data_ptr()
                    pk["struct"] = c
                    self._packed = pk
                fresh = backward and "struct_t" not in pk
                if fresh:
                    pk.update(w2_t=z((HIDDEN_PAD, K), dt), w1_t=z((K, HIDDEN_PAD), dt), inv_w_t=z((2 * K, MAX_ROWS), dt))
                    c = _capi.IcmBwd()
                    c.fwd_w2_t, c.fwd_w1_t, c.inv_w_t = (pk[k].data_ptr() for k in ("w2_t", "w1_t", "inv_w_t"))
                    pk["struct_t"] = c
                if pk["key"] != key or fresh:
                    with torch.no_grad():
                        w1 = fwd.fc1.weight.detach()
                        pk["w1"][:HIDDEN].copy_(w1[:, :K])
                        pk["w1_act"][:, :HIDDEN].copy_(w1[:, K:].t())
                        pk["b1"][:HIDDEN].copy_(fwd.fc1.bias.detach())
                        pk["w2"][:, :HIDDEN].copy_(fwd.fc2.weight.detach())
                        pk["b2"].copy_(fwd.fc2.bias.detach())
                        pk["inv_w"][:N].copy_(torch.cat([l.weight.detach() for l in lin], dim=0))
                        pk["inv_b"][:N].copy_(torch.cat([l.bias.detach() for l in lin], dim=0))
                        if "struct_t" in pk:
                            pk["w2_t"].copy_(pk["w2"].t())
                            pk["w1_t"].copy_(pk["w1"].t())
                            pk["inv_w_t"].copy_(pk["inv_w"].t())
                    pk["key"] = key
                return pk

            def _fused(self, features, actions, agent_finished, want_losses, backward=False):
                T, P, K = features.shape[0] - 1, features.shape[1], features.shape[2]
                G, dev = len(self.groups), features.device
                pk = self._weights(dev, backward)
                curiosity = torch.empty((T, P), dtype=torch.float32, device=dev)
                ce = torch.empty((T, G, P), dtype=torch.float32, device=dev)
                losses = torch.empty((3,), dtype=torch.float32, device=dev) if want_losses else None
                nvec = (C.c_int32 * G)(*self.groups)
                lib, p = _capi.load(), _capi.ptr
                with torch.cuda.device(dev):
                    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    _capi.check(lib.dynenv_icm_losses(p(features), p(actions), p(agent_finished), T, P, K, actions.shape[1], nvec, G,
                                                      _capi.ARR_BF16 if self.w_dtype == torch.bfloat16 else _capi.ARR_F16, C.byref(pk["struct"]),
                                                      float(self.pred_net.fwd_net.relu.negative_slope), p(curiosity), p(ce), p(losses), p(self.status),
                                                      stream), "dynenv_icm_losses")
                return curiosity, ce, losses

            # ---- the fused backward
            def _no_fused_backward(self, features, actions, agent_finished):
                """why dynenv_icm_backward does not take this call, or None"""
                why = self._not_fusable(features, actions, agent_finished)
                if why is None and self.feature_size not in FUSED_BACKWARD_K:
                    why = "K = %d: the fused backward takes 64 or 128" % self.feature_size
                return why

            def _backward_buffers(self, dev, P):
                """the seven gradients in the packed layouts and the workspace: the module's, at fixed addresses (the workspace
                grows with P up to its bound, dynenv.h)"""
                K, N = self.feature_size, sum(self.groups)
                need = C.c_uint64(0)
                _capi.check(_capi.load().dynenv_icm_backward_workspace(P, K, C.byref(need)), "dynenv_icm_backward_workspace")
                b = self._bwd
                if b is None or b["dev"] != dev:
                    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
                    b = dict(dev=dev, w1=e(HIDDEN_PAD, K), act=e(N, HIDDEN_PAD), b1=e(HIDDEN_PAD), w2=e(K, HIDDEN_PAD), b2=e(K), inv_w=e(MAX_ROWS, 2 * K),
                             inv_b=e(MAX_ROWS), ws=None)
                    c = _capi.IcmGrad()
                    c.d_fwd_w1, c.d_fwd_w1_act, c.d_fwd_b1, c.d_fwd_w2, c.d_fwd_b2 = (b[k].data_ptr() for k in ("w1", "act", "b1", "w2", "b2"))
                    c.d_inv_w, c.d_inv_b = b["inv_w"].data_ptr(), b["inv_b"].data_ptr()
                    b["struct"] = c
                    self._bwd = b
                if b["ws"] is None or b["ws"].numel() < need.value:
                    b["ws"] = torch.empty((need.value,), dtype=torch.uint8, device=dev)
                return b

            def _fused_backward(self, features, actions, agent_finished, losses, upstream, want_features, wanted):
                """one call of dynenv_icm_backward -> (d_features or None, the gradients of _params() where `wanted`, else None)"""
                T, P, K = features.shape[0] - 1, features.shape[1], features.shape[2]
                G, dev, pk = len(self.groups), features.device, self._packed
                b = self._backward_buffers(dev, P)
                d_features = torch.empty_like(features) if want_features else None
                nvec = (C.c_int32 * G)(*self.groups)
                lib, p = _capi.load(), _capi.ptr
                with torch.cuda.device(dev):
                    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    _capi.check(lib.dynenv_icm_backward(p(features), p(actions), p(agent_finished), T, P, K, actions.shape[1], nvec, G,
                                                        _capi.ARR_BF16 if self.w_dtype == torch.bfloat16 else _capi.ARR_F16, C.byref(pk["struct"]),
                                                        float(self.pred_net.fwd_net.relu.negative_slope), p(losses), p(upstream), C.byref(pk["struct_t"]),
                                                        C.byref(b["struct"]), p(d_features), p(b["ws"]), b["ws"].numel(), p(self.status), stream),
                                "dynenv_icm_backward")
                starts, sizes = [sum(self.groups[:g]) for g in range(G)], self.groups   # (host ints: nothing is read from the device)
                out =[torch.cat((b["w1"][:HIDDEN, :K], b["act"][:, :HIDDEN].t()), dim=1), b["b1"][:HIDDEN].clone(), b["w2"][:, :HIDDEN].clone(), b["b2"].clone()]
                for s0, n in zip(starts, sizes):
                    out += [b["inv_w"][s0:s0 + n].clone(), b["inv_b"][s0:s0 + n].clone()]
                return d_features, [g if w else None for g, w in zip(out, wanted)]

            def _forward_fused_backward(self, features, actions, agent_finished, long_horizon):
                losses = _function().apply(self, features, actions, agent_finished, *self._params())
                fwd, inv = self.forward_coeff * losses[0], self.icm_beta * losses[1]
                with torch.no_grad():
                    if long_horizon:
                        lh = self._long_horizon(features.detach(), self._one_hot(self._indices(actions), features.dtype), losses[2] > 0)
                    else:
                        lh = torch.zeros((), dtype=torch.float32, device=features.device)
                return ICMLosses(inv + fwd, inv, fwd, lh)

            def _check(self, features, actions, agent_finished):
                G, K = len(self.groups), self.feature_size
                assert features.dim() == 3 and features.shape[0] >= 2 and features.shape[2] == K, "features is [T + 1, P, %d]" % K
                T, P = features.shape[0] - 1, features.shape[1]
                assert actions.dim() == 3 and actions.shape[0] == T and actions.shape[1] >= G and actions.shape[2] == P, \
                    "actions is [%d, AD >= %d, %d]" % (T, G, P)
                assert agent_finished is None or tuple(agent_finished.shape) == (T, P), "agent_finished is [%d, %d]" % (T, P)

            def forward(self, features, actions, agent_finished=None, long_horizon=False):
                self._check(features, actions, agent_finished)
                if torch.is_grad_enabled() and (features.requires_grad or any(p.requires_grad for p in self.parameters())):
                    self._route = "torch"
                    if self.fused_backward:
                        why = self._no_fused_backward(features, actions, agent_finished)
                        if why is None:
                            self._route = "fused (backward)"
                            return self._forward_fused_backward(features, actions, agent_finished, long_horizon)
                        self._route = "torch (fallback: %s)" % why
                    return self._forward_torch(features, actions, agent_finished, long_horizon)
                with torch.no_grad():
                    why = self._not_fusable(features, actions, agent_finished)
                    if why is not None:
                        self._route = "torch (fallback: %s)" % why
                        return self._forward_torch(features, actions, agent_finished, long_horizon)
                    self._route = "fused"
                    _, _, losses = self._fused(features, actions, agent_finished, True)
                    fwd, inv = self.forward_coeff * losses[0], self.icm_beta * losses[1]
                    if long_horizon:
                        lh = self._long_horizon(features, self._one_hot(self._indices(actions), features.dtype), losses[2] > 0)
                    else:
                        lh = torch.zeros((), dtype=torch.float32, device=features.device)
                    return ICMLosses(inv + fwd, inv, fwd, lh)

            def rows(self, features, actions):
                self._check(features, actions, None)
                with torch.no_grad():
                    features, actions = features.detach(), actions.detach()
                    why = self._not_fusable(features, actions, None, for_loss=False)
                    if why is None:
                        self._route = "fused"
                        curiosity, ce, _ = self._fused(features, actions, None, False)
                        return curiosity, ce
                    self._route = "torch (fallback: %s)" % why
                    se, ce, _ = self._rows_torch(features, self._indices(actions))
                    return se.mean(-1).float(), torch.stack(ce, dim=1).float()

        def _function():
            if "fn" not in _lazy:
                class IcmLossesFunction(torch.autograd.Function):
                    """losses [3] = { forward_mean, inverse_mean, n } by dynenv_icm_losses; the gradient by dynenv_icm_backward.  Saved: the
                    inputs and `losses`, nothing else.  The upstream gradient [3] arrives as a device tensor and goes to the kernel as it is:
                    its elements 0 and 1 are s_f and s_i."""

                    @staticmethod
                    def forward(ctx, module, features, actions, agent_finished, *params):
                        with torch.no_grad():
                            _, _, losses = module._fused(features.detach(), actions, agent_finished, True, backward=True)
                        ctx.module = module
                        ctx.save_for_backward(features, actions, agent_finished, losses)
                        return losses

                    @staticmethod
                    @torch.autograd.function.once_differentiable
                    def backward(ctx, grad):
                        features, actions, agent_finished, losses = ctx.saved_tensors
                        need = ctx.needs_input_grad
                        upstream = grad.to(torch.float32).contiguous()
                        d_features, grads = ctx.module._fused_backward(features.detach(), actions, agent_finished, losses, upstream, need[1], need[4:])
                        return (None, d_features, None, None) + tuple(grads)
                _lazy["fn"] = IcmLossesFunction
            return _lazy["fn"]

        for cls in (ForwardNet, AttentionNet, ICMDynamics, LongHorizonCuriosityLoss, LongHorizonForwardNet, GpuICM):
            cls.__qualname__ = cls.__name__
        _lazy["icm"] = {"GpuICM": GpuICM}
    return _lazy["icm"]


def __getattr__(name):
    if name == "GpuICM":
        return _classes()[name]
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
