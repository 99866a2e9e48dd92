"""The layers behind the feature extractor: the reference's policy head - ActorLayer and CriticLayer (DynEnv/models/actor_critic.py:161-242),
the softmax and the draw of A2CNet._calc_log_probs (actor_critic.py:125-140) and transformActions (DynEnv/utils/utils.py:20-39) -
differentiable through torch where a gradient is wanted and ONE kernel (dynenv_policy_head, csrc/policy_kernels.hip) where none is.
Both routes make the SAME draw: Philox4x32-10 keyed by (seed; row, draw counter, group), then the float32 inverse CDF of the
probabilities (include/dynenv.h, dynenv_policy_head) - not torch.multinomial - so an action can be reproduced from the probabilities."""
import collections
import ctypes as C
import os

from . import _capi

M32 = 0xFFFFFFFF
RNG_PURPOSE = 16   # DYNENV_POLICY_RNG_PURPOSE
MAX_ROWS, MAX_GROUPS, MAX_GROUP, MAX_CONT, MAX_COLS = 32, 8, 16, 4, 8   # the kernel's limits (include/dynenv.h)

EVAL_K = (64, 128)                            # what dynenv_policy_eval and its backward take
EVAL_ROWS, EVAL_MAX_WORKGROUPS = 64, 256     # DYNENV_POLICY_EVAL_ROWS, DYNENV_POLICY_EVAL_MAX_WORKGROUPS: the backward's blocks and its grid's cap

PolicyAct = collections.namedtuple("PolicyAct", ["actions", "head", "log_probs", "probs", "value", "next_ext"])
PolicyEval = collections.namedtuple("PolicyEval", ["log_probs", "probs", "values"])


def transform_actions(actions, discrete_turn=False):
    """The reference's transformActions (utils.py:20-39) on a device tensor [P, AD], with no host read (torch.where instead of masked
    assignment) - the function as its in-place assignments run, not a tidied one: with four columns, column 0 maps 0, 1, 2 -> 0,
    3 -> 1, 4 -> -1; column 1 maps 2 -> -1; column 2 is the `sides` of column 0, where 2 -> 1 and then every 1 -> -1, so BOTH 1 and 2
    give -1 and the rest 0; column 3 is lowered by 3 where discrete_turn.  With any other width columns 0 and 1 are lowered by 1 (a
    single column: that one).  Returns a new tensor of the same dtype."""
    import torch
    new = actions.clone()
    if actions.shape[1] == 4:
        a0, a1 = actions[:, 0], actions[:, 1]
        new[:, 0] = torch.where(a0 < 3, 0, torch.where(a0 == 3, 1, torch.where(a0 == 4, -1, a0)))
        new[:, 1] = torch.where(a1 == 2, -1, a1)
        new[:, 2] = torch.where((a0 == 1) | (a0 == 2), -1, 0)
        if discrete_turn:
            new[:, 3] -= 3
    else:
        new[:, :2] -= 1
    return new


def _mul_hi_lo(a, b):
    """the two 32-bit halves of a * b, a < 2^32 a Python int, b < 2^32 an int64 tensor: torch has no unsigned 64-bit product"""
    p_lo, p_hi = (b & 0xFFFF) * a, (b >> 16) * a
    mid = p_hi + (p_lo >> 16)
    return mid >> 16, ((mid & 0xFFFF) << 16) | (p_lo & 0xFFFF)


def philox4x32_10(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 (include/dynenv_math.h, dm_philox) with torch integer ops: the key two Python ints, the counter words int64
    tensors (or Python ints) below 2^32 -> four int64 tensors below 2^32"""
    for r in range(10):
        hi0, lo0 = _mul_hi_lo(0xD2511F53, c0)
        hi1, lo1 = _mul_hi_lo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw_uniform(seed, draw, row_base, P, G, device):
    """u [P, G] float32 in [0, 1), the draw of dynenv_policy_head: for row p and group g the word g % 4 of philox(key = (lo32(seed),
    hi32(seed)), counter = (lo32(row_base + p), lo32(draw), hi32(draw), RNG_PURPOSE + g // 4)), u = (word >> 8) * 2^-24.  `draw` is an
    int64 tensor of one element holding the 64-bit counter's bits: read on the device."""
    import torch
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    rows = (torch.arange(P, dtype=torch.int64, device=device) + (int(row_base) & M32)) & M32
    d = draw.reshape(1).to(device)
    d_lo, d_hi = d & M32, (d >> 32) & M32
    zero = torch.zeros_like(rows)
    cols = []
    for b in range((G + 3) // 4):
        words = philox4x32_10(seed & M32, seed >> 32, rows, d_lo + zero, d_hi + zero, RNG_PURPOSE + b)
        cols += [(w >> 8).to(torch.float32) * (2.0 ** -24) for w in words[:G - 4 * b]]
    return torch.stack(cols, dim=1)


def sample_inverse_cdf(probs, u):
    """probs [P, n], u [P] -> int64 [P]: c_j = c_{j-1} + probs[:, j] summed left to right in probs' type (not torch.cumsum, whose
    order is another), t = u * c_{n-1}, the number of j in 0..n-2 with c_j <= t"""
    import torch
    n = probs.shape[1]
    c, cs = probs[:, 0], []
    for j in range(1, n):
        cs.append(c)
        c = c + probs[:, j]
    t = u.to(probs.dtype) * c
    act = torch.zeros(probs.shape[0], dtype=torch.int64, device=probs.device)
    for cj in cs:
        act = act + (cj <= t).to(torch.int64)
    return act


# torch is imported on first use (the package itself imports without it): the nn.Modules are built then.
_lazy = {}


def _classes():
    if "policy" not in _lazy:
        import torch
        nn = torch.nn

        class ActorBlock(nn.Module):
            """actor_critic.py:176-213: a Box space is one Linear and a sigmoid scaled into [low, high]; a MultiDiscrete one a Linear per group"""

            def __init__(self, features, action_space, device=None):
                super().__init__()
                self.cont = not hasattr(action_space, "nvec")
                if self.cont:
                    import numpy as np
                    self.shape = int(sum(action_space.shape))
                    high, low = np.asarray(action_space.high, np.float32), np.asarray(action_space.low, np.float32)
                    # (the reference keeps these two as plain attributes moved by _apply; buffers outside state_dict() do the same)
                    self.register_buffer("means", torch.tensor((high + low) * 0.5, device=device).reshape(-1), persistent=False)
                    self.register_buffer("scale", torch.tensor((high - low) * 0.5, device=device).reshape(-1), persistent=False)
                    self.Layer = nn.Linear(features, self.shape, device=device)
                    self.activation = nn.Sigmoid()
                else:
                    self.Layer = nn.ModuleList([nn.Linear(features, int(num), device=device) for num in action_space.nvec])

            def forward(self, x):
                if self.cont:
                    return [(self.activation(self.Layer(x)) - 0.5) * self.scale + self.means]
                return [l(x) for l in self.Layer]

        class ActorLayer(nn.Module):
            def __init__(self, features, actions, device=None):
                super().__init__()
                self.blocks = nn.ModuleList([ActorBlock(features, action, device) for action in actions])

            def forward(self, x):
                return [out for block in self.blocks for out in block(x)]

        class CriticBlock(nn.Module):
            def __init__(self, feature_size, out_size, device=None):
                super().__init__()
                self.Layer1 = nn.Linear(feature_size, feature_size // 2, device=device)
                self.Layer2 = nn.Linear(feature_size // 2, out_size, device=device)
                self.relu = nn.LeakyReLU(0.1)
                self.bn = nn.LayerNorm(feature_size // 2, device=device)

            def forward(self, x):
                return self.Layer2(self.bn(self.relu(self.Layer1(x))))

        class CriticLayer(nn.Module):
            def __init__(self, features, device=None):
                super().__init__()
                self.blocks = CriticBlock(features, 1, device)

            def forward(self, x):
                return self.blocks(x)

        class GpuPolicyHead(nn.Module):
            """The reference's policy head, parameter for parameter and name for name: `actor` = ActorLayer(feature_size, action_space)
            and `critic` = CriticLayer(feature_size) (A2CNet's members, actor_critic.py:40, 52), so that the actor.* and critic.* keys
            of an A2CNet.state_dict() load with strict=True.  feature_size is K, the width of cat(features[0:2]); action_space is
            env.action_space, a spaces.Tuple of MultiDiscrete and at most one Box member.

            forward(feature) -> (policies, value): A2CNet.forward's tail (actor_critic.py:91-92), always in torch and differentiable -
            the loss needs it.  policies: the G logit tensors [P, n_g], then, with a Box block, its output [P, C] as ONE entry (the
            reference's flatten iterates over that tensor's rows).

            act(feat0, feat1=None, out_actions=None, row_base=0) -> PolicyAct(actions [P, AD] int32, head float64 [P] (None without a
            Box block; [P, C] where C > 1), log_probs [P, G], probs: a list of G views [P, n_g], value [P, 1], next_ext float32
            [P, AD]) on cat(feat0, feat1): the rollout's step (DynEnv/models/train.py:251-266).  AD = G + C; the columns behind G are 0.
            out_actions: a caller-owned contiguous int32 tensor of P * AD elements on the device, e.g. the static [E, A, AD] action
            tensor of a captured step, that the actions are written into (`actions` is then a view of it).  Only the discrete groups
            are sampled: the Box output is returned as `head`, the continuous action step_flat takes (the reference also runs its
            softmax and Categorical over that output, which with one output "samples" the constant 0).

            THE DRAW.  u of row p and group g is draw_uniform(seed, draw counter, row_base, ...), the action the float32 inverse CDF
            sample_inverse_cdf(probs_g, u).  The counter is a module-owned device tensor of one 64-bit word, advanced by one after
            every act() with an in-place op on the stream; reseed(seed, draw=0) sets both.  row_base is the first row's stream: shards
            of a batch pass their first row.

            Routes; `last_route` names the one the latest act took.
              "torch"  when gradients are enabled and a parameter requires one: torch's operations, differentiable through log_probs
                       and value, the same draw made with torch integer ops on the tensor's device, no host read.
              "fused"  otherwise: one launch.  F (= K, or K / 2 with feat1) of 64 or 128, G <= 8 groups of at most 16, C <= 4,
                       N + C <= 32, AD <= 8, float32 contiguous inputs and parameters on the device.  The 16-bit copies of the two
                       weight matrices (operand_dtype) are made with torch ops on the stream at every call: no host wait.
              "torch (fallback: ...)"  where no gradient is wanted but the kernel does not take the call - DYNENV_POLICY_FUSED=0 in
                       the environment among the reasons.  Nothing is raised.
            The routes differ only by the rounding of the probabilities (16-bit operands on the matrix units, float32 accumulation,
            against float32 throughout).

            evaluate(features, actions, want_probs=True) -> PolicyEval(log_probs [T, G, P], probs [T, P, N], values [T, P]) over a STORED
            rollout: features float32 [T, P, K] (storage.features[:-1]), actions float32 [T, AD, P] (storage.actions), the outputs in
            the storage's layouts - what GpuRolloutStorage.a2c_loss(evaluation=...) takes, so that a rollout collected by a replayed
            graph (which carries no history) trains the actor and the critic.  Per row the statement is act()'s with the stored action
            in place of the draw (include/dynenv.h, dynenv_policy_eval); an action outside its group is clamped to the nearest one and
            ORs bit 0 into `eval_status` (int32 [1], the module's; GpuICM's convention).  Only the discrete groups are evaluated: a
            head with a Box block takes the torch route and the Box block's parameters receive no gradient (the reference's loss gives
            them none either: its softmax over one output is the constant 1).  want_probs=False leaves probs None - a loss that takes
            its action_probs from elsewhere does not pay for [T, P, N] twice.  `last_eval_route` names the route the latest call took:
              "torch"  a gradient is wanted (the default then): torch operations, float32 throughout, differentiable.
              "fused"  no gradient is wanted and the kernel takes the call: one launch of dynenv_policy_eval - dynenv_policy_head's
                       device function, so for the actions act() drew from the same rows and weights the bits are act()'s.
              "fused (backward)"  fused_backward=True and a gradient wanted: the fused forward behind a torch.autograd.Function;
                       loss.backward() is ONE call of dynenv_policy_eval_backward (csrc/policy_eval_kernels.hip), which recomputes the
                       forward per row: nothing is saved but the inputs.  K of 64 or 128.
              "torch (fallback: why)"  otherwise - DYNENV_POLICY_FUSED=0, another K and a Box block among the reasons.  Nothing is raised."""

            def __init__(self, feature_size, action_space, operand_dtype=torch.bfloat16, seed=0, device=None, discrete_turn=False, fused_backward=False):
                super().__init__()
                self.feature_size = int(feature_size)
                self.operand_dtype = operand_dtype
                assert self.operand_dtype in (torch.bfloat16, torch.float16), "operand_dtype is torch.bfloat16 or torch.float16"
                self.discrete_turn = bool(discrete_turn)
                spaces = action_space.spaces if hasattr(action_space, "spaces") else list(action_space)
                self.actor = ActorLayer(self.feature_size, spaces, device=device)
                self.critic = CriticLayer(self.feature_size, device=device)
                boxes = [b for b in self.actor.blocks if b.cont]
                assert len(boxes) <= 1 and (not boxes or self.actor.blocks[-1].cont), "at most one Box member, behind the discrete ones"
                self.nvec = [l.out_features for b in self.actor.blocks if not b.cont for l in b.Layer]
                assert self.nvec, "an action space has a discrete group"
                self.n_cont = boxes[0].shape if boxes else 0
                self.action_cols = len(self.nvec) + self.n_cont
                self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
                self.register_buffer("_draw", torch.zeros(1, dtype=torch.int64, device=device), persistent=False)
                self.register_buffer("eval_status", torch.zeros(1, dtype=torch.int32, device=device), persistent=False)
                self.register_buffer("_last", torch.tensor(self.nvec, dtype=torch.int64, device=device) - 1, persistent=False)
                self.fused_backward = bool(fused_backward)
                self._route = self._eval_route = None
                self._packed = self._bwd = None

            @property
            def last_route(self):
                return self._route

            @property
            def last_eval_route(self):
                return self._eval_route

            def reseed(self, seed, draw=0):
                self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
                d = int(draw) & 0xFFFFFFFFFFFFFFFF
                self._draw.fill_(d - (1 << 64) if d >> 63 else d)

            @property
            def draw(self):
                """the counter's device tensor (int64 [1] holding the 64-bit word)"""
                return self._draw

            def forward(self, feature):
                return self.actor(feature), self.critic(feature)

            def _linears(self):
                return [l for b in self.actor.blocks for l in ([b.Layer] if b.cont else list(b.Layer))]

            def _not_fusable(self, feat0, feat1, out_actions):
                """why the kernel does not take this call, or None"""
                K, G, C = self.feature_size, len(self.nvec), self.n_cont
                F = K // 2 if feat1 is not None else K
                if os.environ.get("DYNENV_POLICY_FUSED", "") == "0":
                    return "DYNENV_POLICY_FUSED=0"
                if F not in (64, 128) or (feat1 is not None and K % 2):
                    return "F = %d, not 64 or 128" % F
                if G > MAX_GROUPS or max(self.nvec) > MAX_GROUP or C > MAX_CONT or sum(self.nvec) + C > MAX_ROWS or self.action_cols > MAX_COLS:
                    return "an action space beyond %d groups of %d, %d continuous outputs, %d rows or %d columns" % (
                        MAX_GROUPS, MAX_GROUP, MAX_CONT, MAX_ROWS, MAX_COLS)
                if not feat0.is_cuda:
                    return "features that are not on the device"
                P = feat0.shape[0]
                for t in [feat0] + ([feat1] if feat1 is not None else []):
                    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (P, F) or t.device != feat0.device:
                        return "features that are not float32, contiguous [%d, %d] and on %s" % (P, F, feat0.device)
                if out_actions is not None and (out_actions.dtype != torch.int32 or not out_actions.is_contiguous() or
                                                out_actions.numel() != P * self.action_cols or out_actions.device != feat0.device):
                    return "an out_actions that is not int32, contiguous, of %d elements and on %s" % (P * self.action_cols, feat0.device)
                for p in list(self.parameters()) + [self._draw]:
                    if (p.dtype != torch.float32 and p is not self._draw) or not p.is_contiguous() or p.device != feat0.device:
                        return "parameters that are not float32, contiguous and on %s" % (feat0.device,)
                return None

            def act(self, feat0, feat1=None, out_actions=None, row_base=0):
                if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
                    self._route = "torch"
                    out = self._act_torch(feat0, feat1, out_actions, row_base)
                else:
                    why = self._not_fusable(feat0, feat1, out_actions)
                    if why is not None:
                        self._route = "torch (fallback: %s)" % why
                        out = self._act_torch(feat0, feat1, out_actions, row_base)
                    else:
                        self._route = "fused"
                        out = self._act_fused(feat0, feat1, out_actions, row_base)
                with torch.no_grad():
                    self._draw.add_(1)
                return out

            def _act_torch(self, feat0, feat1, out_actions, row_base):
                feature = feat0 if feat1 is None else torch.cat((feat0, feat1), dim=1)
                policies, value = self.forward(feature)
                G, C, P = len(self.nvec), self.n_cont, feature.shape[0]
                probs = [torch.softmax(l, dim=-1, dtype=torch.float32 if l.dtype in (torch.bfloat16, torch.float16) else None) for l in policies[:G]]
                with torch.no_grad():
                    u = draw_uniform(self.seed, self._draw, row_base, P, G, feature.device)
                    drawn = [sample_inverse_cdf(p.detach(), u[:, g]) for g, p in enumerate(probs)]
                    actions = torch.zeros((P, self.action_cols), dtype=torch.int32, device=feature.device)
                    actions[:, :G] = torch.stack(drawn, dim=1)
                    if out_actions is not None:
                        out_actions.view(P, self.action_cols).copy_(actions)
                        actions = out_actions.view(P, self.action_cols)
                    next_ext = transform_actions(actions, self.discrete_turn).to(torch.float32)
                logp = []
                for p, a in zip(probs, drawn):   # Categorical(probs).log_prob: the clamp of probs_to_logits
                    eps = torch.finfo(p.dtype).eps
                    logp.append(torch.log(p.gather(1, a.view(P, 1)).clamp(eps, 1 - eps)))
                head = None
                if C:
                    head = policies[G].detach().double()
                    head = head.reshape(P) if C == 1 else head
                return PolicyAct(actions, head, torch.cat(logp, dim=1), probs, value, next_ext)

            def _act_fused(self, feat0, feat1, out_actions, row_base):
                K, G, NC, AD = self.feature_size, len(self.nvec), self.n_cont, self.action_cols
                N, P = sum(self.nvec), feat0.shape[0]
                F = K // 2 if feat1 is not None else K
                dev, dt = feat0.device, self.operand_dtype
                lin, blk = self._linears(), self.critic.blocks
                # the operands: alive until the launch is enqueued (the caching allocator orders their reuse on the stream)
                aw = torch.zeros((MAX_ROWS, K), dtype=dt, device=dev)
                aw[:N + NC] = torch.cat([l.weight.detach() for l in lin], dim=0)
                ab = torch.zeros((MAX_ROWS,), dtype=torch.float32, device=dev)
                ab[:N + NC] = torch.cat([l.bias.detach() for l in lin], dim=0)
                w1 = blk.Layer1.weight.detach().to(dt)
                keep = [aw, ab, w1]
                w = _capi.Policy()
                w.actor_w, w.actor_b, w.critic_w1 = aw.data_ptr(), ab.data_ptr(), w1.data_ptr()
                w.critic_b1, w.critic_ln_w, w.critic_ln_b = blk.Layer1.bias.data_ptr(), blk.bn.weight.data_ptr(), blk.bn.bias.data_ptr()
                w.critic_w2, w.critic_b2 = blk.Layer2.weight.data_ptr(), blk.Layer2.bias.data_ptr()
                cont = None
                if NC:
                    box = self.actor.blocks[-1]
                    keep += [box.scale.to(torch.float32).contiguous(), box.means.to(torch.float32).contiguous()]
                    w.cont_scale, w.cont_mean = keep[-2].data_ptr(), keep[-1].data_ptr()
                    cont = torch.empty((P, NC), dtype=torch.float64, device=dev)
                actions = torch.empty((P, AD), dtype=torch.int32, device=dev) if out_actions is None else out_actions.view(P, AD)
                probs = torch.empty((P, N), dtype=torch.float32, device=dev)
                logp = torch.empty((P, G), dtype=torch.float32, device=dev)
                value = torch.empty((P, 1), dtype=torch.float32, device=dev)
                next_ext = torch.empty((P, AD), dtype=torch.float32, device=dev)
                nvec = (C.c_int32 * G)(*self.nvec)
                lib = _capi.load()
                with torch.cuda.device(dev):
                    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    _capi.check(lib.dynenv_policy_head(_capi.ptr(feat0), _capi.ptr(feat1), P, 1, F, 1 if dt == torch.bfloat16 else 2, C.byref(w), nvec,
                                                       G, NC, AD, self.seed, _capi.ptr(self._draw), int(row_base) & 0xFFFFFFFFFFFFFFFF,
                                                       float(blk.relu.negative_slope), float(blk.bn.eps), int(self.discrete_turn),
                                                       _capi.ptr(actions), _capi.ptr(cont), _capi.ptr(probs), _capi.ptr(logp), _capi.ptr(value),
                                                       _capi.ptr(next_ext), stream), "dynenv_policy_head")
                head = None if cont is None else (cont.view(P) if NC == 1 else cont)
                return PolicyAct(actions, head, logp, list(torch.split(probs, self.nvec, dim=1)), value, next_ext)

            # ---- evaluate: the head over a stored rollout
            def _eval_indices(self, actions):
                """actions [T, AD, P] -> int64 [T, G, P] inside the groups; a value that had to be clamped sets the status bit"""
                G = len(self.nvec)
                with torch.no_grad():
                    v = actions[:, :G].detach().round()
                    last = self._last.to(v.dtype).view(1, G, 1)
                    ok = (v >= 0) & (v <= last)
                    idx = torch.where(ok, v, torch.where(v > last, last, torch.zeros_like(v))).long()
                    self.eval_status.bitwise_or_((~ok).any().to(torch.int32))
                return idx

            def _eval_torch(self, features, actions, want_probs):
                G = len(self.nvec)
                idx = self._eval_indices(actions)
                policies, value = self.forward(features)
                wide = lambda x: x.float() if x.dtype in (torch.bfloat16, torch.float16) else x   # noqa: E731
                probs = [torch.softmax(wide(l), dim=-1) for l in policies[:G]]
                logp = []
                eps = torch.finfo(torch.float32).eps   # (float32's in every type: the statement of dynenv_policy_eval)
                for g, p in enumerate(probs):   # Categorical(probs).log_prob: the clamp of probs_to_logits
                    logp.append(torch.log(p.gather(2, idx[:, g].unsqueeze(-1)).squeeze(-1).clamp(eps, 1 - eps)))
                return PolicyEval(torch.stack(logp, dim=1), torch.cat(probs, dim=2) if want_probs else None, wide(value).squeeze(-1))

            def _no_eval_fused(self, features, actions, backward):
                """why dynenv_policy_eval (and, with `backward`, dynenv_policy_eval_backward) does not take this call, or None"""
                K, G = self.feature_size, len(self.nvec)
                if os.environ.get("DYNENV_POLICY_FUSED", "") == "0":
                    return "DYNENV_POLICY_FUSED=0"
                if self.n_cont:
                    return "a Box block"
                if K not in EVAL_K:
                    return "K = %d, not 64 or 128" % K
                if G > MAX_GROUPS or max(self.nvec) > MAX_GROUP or sum(self.nvec) > MAX_ROWS or actions.shape[1] > MAX_COLS:
                    return "an action space beyond %d groups of %d, %d rows or %d columns" % (MAX_GROUPS, MAX_GROUP, MAX_ROWS, MAX_COLS)
                if not features.is_cuda:
                    return "features that are not on the device"
                dev = features.device
                for name, t in (("features", features), ("actions", actions)):
                    if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.data_ptr() % 16:
                        return "%s that is not float32, contiguous, 16-byte aligned and on %s" % (name, dev)
                if features.shape[0] * features.shape[1] > 1 << 30:
                    return "more than 2^30 rows"
                for p in self._eval_params() + [self.eval_status]:
                    if (p.dtype != torch.float32 and p is not self.eval_status) or p.device != dev:
                        return "parameters that are not float32 and on %s" % (dev,)
                return None

            def _eval_params(self):
                """the parameters of the discrete groups and of the critic in the order the fused backward returns their gradients"""
                blk = self.critic.blocks
                return [q for l in self._linears()[:len(self.nvec)] for q in (l.weight, l.bias)] + \
                       [blk.Layer1.weight, blk.Layer1.bias, blk.bn.weight, blk.bn.bias, blk.Layer2.weight, blk.Layer2.bias]

            def _eval_weights(self, dev, backward=False):
                """the packed operands of dynenv_policy_t, made once per device and refreshed in place when a parameter changed; with
                `backward` (and from then on) the transposed bf16 copies of dynenv_policy_bwd_t too, refreshed in the same pass"""
                K, N, dt = self.feature_size, sum(self.nvec), self.operand_dtype
                lin, blk = self._linears()[:len(self.nvec)], self.critic.blocks
                params = self._eval_params()
                key = tuple((p.data_ptr(), p._version) for p in params)
                pk = self._packed
                z = lambda shape, d: torch.zeros(shape, dtype=d, device=dev)   # noqa: E731
                if pk is None or pk["dev"] != dev or pk["dt"] != dt:
                    pk = dict(dev=dev, dt=dt, key=None, aw=z((MAX_ROWS, K), dt), ab=z((MAX_ROWS,), torch.float32), w1=z((K // 2, K), dt))
                    self._packed = pk
                fresh = backward and "aw_t" not in pk
                if fresh:
                    pk.update(aw_t=z((K, MAX_ROWS), torch.bfloat16), w1_t=z((K, K // 2), torch.bfloat16), aw_t_lo=z((K, MAX_ROWS), torch.bfloat16),
                              w1_t_lo=z((K, K // 2), torch.bfloat16))   # (the second halves: read with float16 operands only)
                    c = _capi.PolicyBwd()
                    c.actor_w_t, c.critic_w1_t, c.actor_w_t_lo, c.critic_w1_t_lo = (pk[k].data_ptr() for k in ("aw_t", "w1_t", "aw_t_lo", "w1_t_lo"))
                    pk["struct_t"] = c
                if pk["key"] != key or fresh:
                    with torch.no_grad():
                        pk["aw"][:N].copy_(torch.cat([l.weight.detach() for l in lin], dim=0))
                        pk["ab"][:N].copy_(torch.cat([l.bias.detach() for l in lin], dim=0))
                        pk["w1"].copy_(blk.Layer1.weight.detach())
                        if "aw_t" in pk:
                            for name, w in (("aw_t", torch.cat([l.weight.detach() for l in lin], dim=0).t()), ("w1_t", blk.Layer1.weight.detach().t())):
                                hi = pk[name][:, :w.shape[1]]
                                hi.copy_(w)
                                pk[name + "_lo"][:, :w.shape[1]].copy_(w - hi.float())
                    pk["key"] = key
                w = _capi.Policy()   # (the float32 operands are the parameters themselves: their pointers are read at every call)
                w.actor_w, w.actor_b, w.critic_w1 = pk["aw"].data_ptr(), pk["ab"].data_ptr(), pk["w1"].data_ptr()
                w.critic_b1, w.critic_ln_w, w.critic_ln_b = blk.Layer1.bias.data_ptr(), blk.bn.weight.data_ptr(), blk.bn.bias.data_ptr()
                w.critic_w2, w.critic_b2 = blk.Layer2.weight.data_ptr(), blk.Layer2.bias.data_ptr()
                pk["struct"] = w
                return pk

            def _eval_fused(self, features, actions, want_probs, backward=False):
                T, P, K = features.shape
                G, N, dev, blk = len(self.nvec), sum(self.nvec), features.device, self.critic.blocks
                pk = self._eval_weights(dev, backward)
                logp = torch.empty((T, G, P), dtype=torch.float32, device=dev)
                probs = torch.empty((T, P, N), dtype=torch.float32, device=dev) if want_probs else None
                values = torch.empty((T, P), dtype=torch.float32, device=dev)
                nvec = (C.c_int32 * G)(*self.nvec)
                lib, p = _capi.load(), _capi.ptr
                with torch.cuda.device(dev):
                    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    _capi.check(lib.dynenv_policy_eval(p(features), p(actions), T, P, K, _capi.ARR_BF16 if self.operand_dtype == torch.bfloat16 else _capi.ARR_F16,
                                                       C.byref(pk["struct"]), nvec, G, actions.shape[1], float(blk.relu.negative_slope), float(blk.bn.eps),
                                                       p(logp), p(probs), p(values), p(self.eval_status), stream), "dynenv_policy_eval")
                return logp, probs, values

            def _eval_backward_buffers(self, dev, rows):
                """the eight gradients in the packed layouts and the workspace: the module's, at fixed addresses (the workspace grows
                with the rows up to its bound, dynenv.h)"""
                K = self.feature_size
                need = C.c_uint64(0)
                _capi.check(_capi.load().dynenv_policy_eval_backward_workspace(rows, K, C.byref(need)), "dynenv_policy_eval_backward_workspace")
                b = self._bwd
                if b is None or b["dev"] != dev:
                    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
                    b = dict(dev=dev, aw=e(MAX_ROWS, K), ab=e(MAX_ROWS), w1=e(K // 2, K), b1=e(K // 2), lnw=e(K // 2), lnb=e(K // 2), w2=e(K // 2), b2=e(1),
                             ws=None)
                    c = _capi.PolicyGrad()
                    c.d_actor_w, c.d_actor_b, c.d_critic_w1, c.d_critic_b1 = (b[k].data_ptr() for k in ("aw", "ab", "w1", "b1"))
                    c.d_critic_ln_w, c.d_critic_ln_b, c.d_critic_w2, c.d_critic_b2 = (b[k].data_ptr() for k in ("lnw", "lnb", "w2", "b2"))
                    b["struct"] = c
                    self._bwd = b
                if b["ws"] is None or b["ws"].numel() < need.value:
                    b["ws"] = torch.empty((need.value,), dtype=torch.uint8, device=dev)
                return b

            def _eval_fused_backward(self, features, actions, d_logp, d_probs, d_values, want_features, wanted):
                """one call of dynenv_policy_eval_backward -> (d_features or None, the gradients of _eval_params() where `wanted`, else None)"""
                T, P, K = features.shape
                G, dev, blk = len(self.nvec), features.device, self.critic.blocks
                pk = self._eval_weights(dev, True)
                b = self._eval_backward_buffers(dev, T * P)
                d_features = torch.empty_like(features) if want_features else None
                nvec = (C.c_int32 * G)(*self.nvec)
                lib, p = _capi.load(), _capi.ptr
                with torch.cuda.device(dev):
                    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    _capi.check(lib.dynenv_policy_eval_backward(p(features), p(actions), T, P, K, _capi.ARR_BF16 if self.operand_dtype == torch.bfloat16 else _capi.ARR_F16,
                                                                C.byref(pk["struct"]), nvec, G, actions.shape[1], float(blk.relu.negative_slope), float(blk.bn.eps),
                                                                p(d_logp), p(d_probs), p(d_values), C.byref(pk["struct_t"]), C.byref(b["struct"]), p(d_features),
                                                                p(b["ws"]), b["ws"].numel(), p(self.eval_status), stream), "dynenv_policy_eval_backward")
                out, s0 = [], 0
                for n in self.nvec:   # (host ints: nothing is read from the device)
                    out += [b["aw"][s0:s0 + n].clone(), b["ab"][s0:s0 + n].clone()]
                    s0 += n
                out += [b["w1"].clone(), b["b1"].clone(), b["lnw"].clone(), b["lnb"].clone(), b["w2"].view(1, -1).clone(), b["b2"].clone()]
                return d_features, [g if w else None for g, w in zip(out, wanted)]

            def evaluate(self, features, actions, want_probs=True):
                K, G = self.feature_size, len(self.nvec)
                assert features.dim() == 3 and features.shape[2] == K, "features is [T, P, %d]" % K
                T, P = features.shape[0], features.shape[1]
                assert actions.dim() == 3 and actions.shape[0] == T and actions.shape[1] >= G and actions.shape[2] == P, \
                    "actions is [%d, AD >= %d, %d]" % (T, G, P)
                if torch.is_grad_enabled() and (features.requires_grad or any(p.requires_grad for p in self.parameters())):
                    self._eval_route = "torch"
                    if self.fused_backward:
                        why = self._no_eval_fused(features, actions, True)
                        if why is None:
                            self._eval_route = "fused (backward)"
                            out = _eval_function().apply(self, features, actions, bool(want_probs), *self._eval_params())
                            return PolicyEval(out[0], out[2] if want_probs else None, out[1])
                        self._eval_route = "torch (fallback: %s)" % why
                    return self._eval_torch(features, actions, want_probs)
                with torch.no_grad():
                    why = self._no_eval_fused(features, actions, False)
                    if why is not None:
                        self._eval_route = "torch (fallback: %s)" % why
                        return self._eval_torch(features, actions, want_probs)
                    self._eval_route = "fused"
                    logp, probs, values = self._eval_fused(features, actions, want_probs)
                    return PolicyEval(logp, probs, values)

        def _eval_function():
            if "fn" not in _lazy:
                class PolicyEvalFunction(torch.autograd.Function):
                    """(log_probs, values[, probs]) by dynenv_policy_eval; the gradient by dynenv_policy_eval_backward.  Saved: the inputs,
                    nothing else.  The upstream gradients arrive as device tensors and go to the kernel as they are; one that is missing
                    (an output the loss did not use) is zeros - for probs: NULL."""

                    @staticmethod
                    def forward(ctx, module, features, actions, want_probs, *params):
                        with torch.no_grad():
                            logp, probs, values = module._eval_fused(features.detach(), actions, want_probs, backward=True)
                        ctx.module = module
                        ctx.save_for_backward(features, actions)
                        ctx.set_materialize_grads(False)
                        return (logp, values, probs) if want_probs else (logp, values)

                    @staticmethod
                    @torch.autograd.function.once_differentiable
                    def backward(ctx, d_logp, d_values, d_probs=None):
                        features, actions = ctx.saved_tensors
                        need = ctx.needs_input_grad
                        T, P, _ = features.shape
                        f32 = lambda g, shape: torch.zeros(shape, dtype=torch.float32, device=features.device) if g is None \
                            else g.to(torch.float32).contiguous()   # noqa: E731
                        d_logp, d_values = f32(d_logp, (T, len(ctx.module.nvec), P)), f32(d_values, (T, P))
                        d_probs = None if d_probs is None else d_probs.to(torch.float32).contiguous()
                        d_features, grads = ctx.module._eval_fused_backward(features.detach(), actions, d_logp, d_probs, d_values, need[1], need[4:])
                        return (None, d_features, None, None) + tuple(grads)
                _lazy["fn"] = PolicyEvalFunction
            return _lazy["fn"]

        for cls in (ActorBlock, ActorLayer, CriticBlock, CriticLayer, GpuPolicyHead):
            cls.__qualname__ = cls.__name__
        _lazy["policy"] = {"GpuPolicyHead": GpuPolicyHead, "ActorLayer": ActorLayer, "CriticLayer": CriticLayer}
    return _lazy["policy"]


def __getattr__(name):
    if name in ("GpuPolicyHead", "ActorLayer", "CriticLayer"):
        return _classes()[name]
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
