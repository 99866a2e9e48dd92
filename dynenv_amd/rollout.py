"""What keeps a rollout: the reference's RolloutStorage (DynEnv/models/storage.py) on the device, behind the policy head.  One launch
(dynenv_rollout_insert, csrc/rollout_kernels.hip) inserts a step's results at a row read from a device cursor, so it records into the same
graph as the step; one launch (dynenv_rollout_returns) computes the returns; a2c_loss is the reference's function in torch on the stored
tensors.  GpuRollout composes step, extractor, policy and insert (DynEnv/models/train.py:241-293)."""
import collections
import ctypes as C
import os

from . import _capi

MAX_GROUPS, MAX_COLS, MAX_PROBS = 8, 8, 32   # the insert kernel's limits, dynenv_policy_head's (include/dynenv.h)
RETURN_MODES = {"reference": _capi.RETURNS_REFERENCE, "dones": _capi.RETURNS_DONES, "gae": _capi.RETURNS_GAE}

A2CLosses = collections.namedtuple("A2CLosses", ["loss", "policy", "value", "entropy", "temp_entropy", "rewards"])


def returns_torch(rewards, values, dones, final_value, num_players, discount=0.99, mode="reference", gae_lambda=0.95):
    """The operations of dynenv_rollout_returns (include/dynenv.h) as torch statements, float32, one rounding per multiply and add in
    the header's order -> (returns, advantages), both [T, P].  Mode "reference" is _discount_rewards (storage.py:168-209) as it runs:
    the Python scalar `discount` multiplies a float32 tensor as float32(discount), and dones are not looked at."""
    import numpy as np
    import torch
    T, P = rewards.shape
    g = float(np.float32(discount))
    gl = float(np.float32(discount) * np.float32(gae_lambda))
    ret, adv_out = torch.zeros_like(rewards), torch.zeros_like(rewards)
    with torch.no_grad():
        values, final = values.detach(), final_value.detach().reshape(-1).to(rewards.dtype)
        nd = None
        if mode != "reference":
            nd = (1 - dones).view(T, -1, 1).expand(T, dones.shape[1], num_players).reshape(T, P)
        if mode == "gae":
            adv, nxt = torch.zeros_like(final), final
            for t in reversed(range(T)):
                delta = (rewards[t] + (g * nxt) * nd[t]) - values[t]
                adv = delta + (gl * adv) * nd[t]
                ret[t].copy_(adv + values[t])
                adv_out[t].copy_(adv)
                nxt = values[t]
            return ret, adv_out
        R = final
        for t in reversed(range(T)):
            R = rewards[t] + g * R if mode == "reference" else rewards[t] + (g * R) * nd[t]
            ret[t].copy_(R)
        return ret, ret - values


class GpuRolloutStorage(object):
    """The reference's RolloutStorage under its attribute names, shapes and dtypes (reset_buffers, storage.py:76-111), P = num_envs *
    num_players: rewards [T, P], agentFinished bool [T, P], features [T + 1, P, feature_size], actions [T, action_cols, P], log_probs
    (and, with use_ppo, log_probs_old) [T, G, P], values [T, P], dones [T, num_envs], all float32 but agentFinished; and - where the
    reference keeps a Python list of the steps' action_probs (train.py:257) - probs [T, P, n_probs] when n_probs > 0.  `groups` is the
    tuple of the discrete groups' sizes (GpuPolicyHead.nvec), G = len(groups); n_probs is 0 or sum(groups).

    The row of an insert is `cursor`, an int32 [1] on the device that insert() advances with an in-place op on the stream, so that
    insert() records into a graph; `status` (int32 [1]) becomes 1 when an insert found the cursor outside the rollout - such an
    insert writes nothing else - and stays 1 until after_update().

    insert(rewards, finished, feat0, feat1, actions, log_probs, value, dones, probs=None, log_probs_old=None) is storage.py:134-166 for
    the tensors a step and GpuPolicyHead.act leave on the device: rewards float64 [E, A], finished bool / uint8 [E, A] (BatchedDynEnv.
    agent_finished()), feat0 and feat1 (or None) float32 [P, F] - stored side by side, the reference's cat -, actions int32 [P, AD],
    log_probs float32 [P, G], value float32 [P] or [P, 1], dones uint8 / bool [E], probs float32 [P, N] or the list of its G column
    blocks.  Routes; `last_route` names the one the latest insert took:
      "fused"  no argument carries a gradient and the kernel takes the call: one launch.
      "torch"  one does: the reference's copy_ statements at the cursor, through index_copy_ with the device cursor: still capturable,
               and differentiable as the reference's storage is.
      "torch (fallback: why)"  otherwise - DYNENV_ROLLOUT_FUSED=0 in the environment among the reasons.  Nothing is raised.
    The routes perform no arithmetic that could differ: their results are identical bit for bit."""

    def __init__(self, rollout_size, num_envs, num_players, action_cols, groups, feature_size, n_probs=0, use_full_entropy=False, use_ppo=False,
                 ppo_clip=0.2, device=None):
        import torch
        self.rollout_size, self.num_envs, self.num_players = int(rollout_size), int(num_envs), int(num_players)
        self.num_all_players = self.num_envs * self.num_players
        self.action_cols, self.groups, self.feature_size, self.n_probs = int(action_cols), tuple(int(n) for n in groups), int(feature_size), int(n_probs)
        self.num_actions = len(self.groups)
        assert self.rollout_size >= 1 and self.num_envs >= 1 and self.num_players >= 1 and self.feature_size >= 1
        assert 1 <= self.num_actions <= self.action_cols, "action_cols is at least the number of groups"
        assert self.n_probs in (0, sum(self.groups)), "n_probs is 0 or sum(groups)"
        self.use_full_entropy, self.use_ppo, self.ppo_clip = bool(use_full_entropy), bool(use_ppo), ppo_clip
        if device is None:
            device = "cuda:%d" % torch.cuda.current_device() if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        T, E, P, G = self.rollout_size, self.num_envs, self.num_all_players, self.num_actions
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.rewards = z(T, P)
        self.agentFinished = torch.zeros((T, P), dtype=torch.bool, device=self.device)
        self.features = z(T + 1, P, self.feature_size)
        self.actions = z(T, self.action_cols, P)
        self.log_probs = z(T, G, P)
        self.log_probs_old = z(T, G, P) if self.use_ppo else None
        self.values = z(T, P)
        self.dones = z(T, E)
        self.probs = z(T, P, self.n_probs) if self.n_probs else None
        self.cursor = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._route = self._returns_route = None

    @property
    def last_route(self):
        return self._route

    @property
    def last_returns_route(self):
        return self._returns_route

    _BUFFERS = ("rewards", "agentFinished", "features", "actions", "log_probs", "log_probs_old", "values", "dones", "probs")

    def buffers(self):
        """name -> tensor of the buffers the storage has"""
        return {k: getattr(self, k) for k in self._BUFFERS if getattr(self, k) is not None}

    def after_update(self):
        """Rewinds the cursor, clears the status word and zeroes the buffers IN PLACE.  This differs deliberately from the reference's
        after_update (storage.py:113-122), which allocates new tensors: here the pointers stay fixed, so a recorded graph that inserts
        into them stays valid.  A buffer that took part in a backward pass is detached first (same memory): what the reference frees by
        dropping the tensor."""
        import torch
        with torch.no_grad():
            for k, b in self.buffers().items():
                if b.grad_fn is not None or b.requires_grad:
                    b = b.detach()
                    setattr(self, k, b)
                b.zero_()
            self.cursor.zero_()
            self.status.zero_()

    # ---- insert
    def _probs_tensor(self, probs):
        """[P, N]: the tensor itself, the tensor the G column blocks are views of (GpuPolicyHead's fused route), or their cat"""
        import torch
        if probs is None or isinstance(probs, torch.Tensor):
            return probs
        base = probs[0]._base
        if base is not None and base.dim() == 2 and base.shape[1] == sum(p.shape[1] for p in probs) and base.is_contiguous() and \
                all(p._base is base for p in probs) and [p.storage_offset() - base.storage_offset() for p in probs] == \
                [sum(q.shape[1] for q in probs[:i]) for i in range(len(probs))] and not any(p.requires_grad for p in probs):
            return base
        return torch.cat(list(probs), dim=1)

    def _check(self, rewards, finished, feat0, feat1, actions, log_probs, value, dones, probs, log_probs_old):
        E, P, G = self.num_envs, self.num_all_players, self.num_actions
        F = self.feature_size // 2 if feat1 is not None else self.feature_size
        assert feat1 is None or self.feature_size % 2 == 0
        for name, t, n in (("rewards", rewards, P), ("finished", finished, P), ("value", value, P), ("dones", dones, E)):
            assert t is None or t.numel() == n, "%s has %d elements, not %d" % (name, t.numel(), n)
        for name, t, cols in (("feat0", feat0, F), ("feat1", feat1, F), ("actions", actions, self.action_cols), ("log_probs", log_probs, G),
                              ("log_probs_old", log_probs_old, G), ("probs", probs, self.n_probs)):
            assert t is None or tuple(t.shape) == (P, cols), "%s is %s, not [%d, %d]" % (name, tuple(t.shape), P, cols)
        assert probs is None or self.probs is not None, "probs given to a storage made with n_probs = 0"
        assert log_probs_old is None or self.log_probs_old is not None, "log_probs_old given to a storage made with use_ppo = False"
        return F

    def _not_fusable(self, F, tensors):
        """why the kernel does not take this call, or None.  tensors: (name, tensor or None, dtypes)"""
        import torch
        if os.environ.get("DYNENV_ROLLOUT_FUSED", "") == "0":
            return "DYNENV_ROLLOUT_FUSED=0"
        if self.device.type != "cuda":
            return "a storage that is not on the device"
        if F % 4:
            return "F = %d, not a multiple of 4" % F
        if self.num_actions > MAX_GROUPS or self.action_cols > MAX_COLS or self.n_probs > MAX_PROBS:
            return "a storage beyond %d groups, %d action columns or %d probabilities" % (MAX_GROUPS, MAX_COLS, MAX_PROBS)
        for name, t, dtypes in tensors:
            if t is not None and (t.dtype not in dtypes or not t.is_contiguous() or t.device != self.device):
                return "%s that is not %s, contiguous and on %s" % (name, " / ".join(str(d) for d in dtypes), self.device)
            if t is not None and name in ("feat0", "feat1") and t.data_ptr() % 16:
                return "%s that is not 16-byte aligned" % name
        return None

    def insert(self, rewards, finished, feat0, feat1, actions, log_probs, value, dones, probs=None, log_probs_old=None):
        import torch
        probs = self._probs_tensor(probs)
        F = self._check(rewards, finished, feat0, feat1, actions, log_probs, value, dones, probs, log_probs_old)
        args = (rewards, finished, feat0, feat1, actions, log_probs, value, dones, probs, log_probs_old)
        self._insert(F, args, features_only=False)
        with torch.no_grad():
            self.cursor.add_(1)

    def insert_final(self, feat0, feat1=None):
        """features[T] = cat(feat0, feat1): the reference's features[step + 1].copy_(final_features) (train.py:290).  The cursor stands
        at T after rollout_size inserts and stays there."""
        F = self._check(None, None, feat0, feat1, None, None, None, None, None, None)
        self._insert(F, (None, None, feat0, feat1, None, None, None, None, None, None), features_only=True)

    def _insert(self, F, args, features_only):
        import torch
        rewards, finished, feat0, feat1, actions, log_probs, value, dones, probs, log_probs_old = args
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in args):
            self._route = "torch"
            return self._insert_torch(args, features_only)
        b8 = (torch.bool, torch.uint8)
        why = self._not_fusable(F, (("rewards", rewards, (torch.float64,)), ("finished", finished, b8), ("feat0", feat0, (torch.float32,)),
                                    ("feat1", feat1, (torch.float32,)), ("actions", actions, (torch.int32,)), ("log_probs", log_probs, (torch.float32,)),
                                    ("value", value, (torch.float32,)), ("dones", dones, b8), ("probs", probs, (torch.float32,)),
                                    ("log_probs_old", log_probs_old, (torch.float32,))))
        if why is None:
            for k, b in self.buffers().items():   # (a buffer that a differentiable insert wrote is a view of the graph: the kernel leaves it alone)
                if b.grad_fn is not None:
                    why = "a %s that carries a gradient: after_update() first" % k
                    break
        if why is not None:
            self._route = "torch (fallback: %s)" % why
            return self._insert_torch(args, features_only)
        self._route = "fused"
        lib, p = _capi.load(), _capi.ptr
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _capi.check(lib.dynenv_rollout_insert(
                p(self.cursor), self.rollout_size, self.num_envs, self.num_players, F, self.num_actions, self.action_cols, self.n_probs, int(features_only),
                p(rewards), p(finished), p(feat0), p(feat1), p(actions), p(log_probs), p(log_probs_old), p(value), p(dones), p(probs),
                p(self.rewards), p(self.agentFinished), p(self.features), p(self.actions), p(self.log_probs), p(self.log_probs_old), p(self.values),
                p(self.dones), p(self.probs), p(self.status), stream), "dynenv_rollout_insert")

    def _insert_torch(self, args, features_only):
        """storage.py:158-166, each copy_ at the row the device cursor names: index_copy_ with the cursor as its index.  A cursor outside
        the rollout must write nothing (and an index outside a tensor is a device fault), so the index is clamped and, where it was
        outside, the row is written with what it held."""
        import torch
        rewards, finished, feat0, feat1, actions, log_probs, value, dones, probs, log_probs_old = args
        T, E, P = self.rollout_size, self.num_envs, self.num_all_players
        last = T if features_only else T - 1
        with torch.no_grad():
            ok = (self.cursor >= 0) & (self.cursor <= last)
            idx = self.cursor.clamp(0, last).long()
            self.status.copy_(torch.where(ok, self.status, torch.ones_like(self.status)))

        def put(name, row):
            buf = getattr(self, name)
            row = row.unsqueeze(0)
            row = torch.where(ok.view((1,) * row.dim()), row, buf.index_select(0, idx))
            buf.index_copy_(0, idx, row)

        if feat0 is not None:
            put("features", feat0 if feat1 is None else torch.cat((feat0, feat1), dim=1))
        if features_only:
            return
        if rewards is not None:
            put("rewards", rewards.reshape(P).to(torch.float32))
        if finished is not None:
            put("agentFinished", finished.reshape(P) != 0)
        if actions is not None:
            put("actions", actions.t().to(torch.float32))
        if log_probs is not None:
            put("log_probs", log_probs.t())
        if log_probs_old is not None:
            put("log_probs_old", log_probs_old.t())
        if value is not None:
            put("values", value.reshape(P))
        if dones is not None:
            put("dones", (dones.reshape(E) != 0).to(torch.float32))
        if probs is not None:
            put("probs", probs)

    # ---- returns and the loss
    def returns(self, final_value, discount=0.99, mode="reference", gae_lambda=0.95):
        """-> (returns, advantages), float32 [T, P], without a gradient (the reference's chain has none: final_value comes from a
        no_grad block, train.py:284-288).  mode "reference" is _discount_rewards (storage.py:168-209) as it runs - dones are not looked
        at -, "dones" cuts the chain where an episode ended, "gae" is generalised advantage estimation; include/dynenv.h,
        dynenv_rollout_returns, states the order of operations.  One launch where the tensors are float32, contiguous and on the device
        (`last_returns_route` "fused"), the torch statements of the same operations otherwise: both are bit-identical."""
        import numpy as np
        import torch
        assert mode in RETURN_MODES, "mode is one of %s" % (sorted(RETURN_MODES),)
        T, E, A, P = self.rollout_size, self.num_envs, self.num_players, self.num_all_players
        assert final_value.numel() == P
        rewards, values, dones, final = self.rewards.detach(), self.values.detach(), self.dones.detach(), final_value.detach().reshape(-1)
        why = None
        if os.environ.get("DYNENV_ROLLOUT_FUSED", "") == "0":
            why = "DYNENV_ROLLOUT_FUSED=0"
        elif self.device.type != "cuda":
            why = "a storage that is not on the device"
        elif final.dtype != torch.float32 or not final.is_contiguous() or final.device != self.device:
            why = "a final_value that is not float32, contiguous and on %s" % (self.device,)
        if why is not None:
            self._returns_route = "torch (fallback: %s)" % why
            return returns_torch(rewards, values, dones, final, A, discount, mode, gae_lambda)
        self._returns_route = "fused"
        ret, adv = torch.empty_like(rewards), torch.empty_like(rewards)
        lib, p = _capi.load(), _capi.ptr
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _capi.check(lib.dynenv_rollout_returns(p(rewards), p(values), p(dones), p(final), T, E, A, RETURN_MODES[mode], float(np.float32(discount)),
                                                   float(np.float32(gae_lambda)), p(ret), p(adv), stream), "dynenv_rollout_returns")
        return ret, adv

    def _ppo_loss(self, advantage, log_probs, delta=1e-8):
        """storage.py:264-290 as it runs: `+ delta` stands outside the exp, and the minimum is returned with the sign it has"""
        import torch
        r_theta = torch.stack([torch.exp(log_prob - old_log_prob) + delta for log_prob, old_log_prob in
                               zip(log_probs.permute(1, 0, 2), self.log_probs_old.permute(1, 0, 2))])
        r_theta_clipped = torch.clamp(r_theta, 1 - self.ppo_clip, 1 + self.ppo_clip)
        ppo_loss, _ = torch.min(torch.stack((r_theta * advantage.detach(), r_theta_clipped * advantage.detach())), dim=0)
        return ppo_loss.mean()

    def a2c_loss(self, final_values, action_probs=None, value_coeff=0.5, entropy_coeff=0.1, discount=0.99, mode="reference", gae_lambda=0.95,
                 evaluation=None):
        """The reference's a2c_loss (storage.py:211-262) statement for statement in torch on the stored tensors - the function as it
        runs, not a tidied one.  The returns come from returns(): `advantage = returns - values` differentiates through `values` alone,
        as the reference's does; with mode "gae" the policy term is weighted by returns()'s advantages instead.  action_probs: the
        reference's list over the steps of the list of the G probability tensors [P, n_g], or None for the stored `probs`.
        evaluation: a PolicyEval (GpuPolicyHead.evaluate on features[:-1] and actions) whose log_probs, values and probs stand where the
        stored log_probs, values and probs stood in the loss's statements - a rollout collected by a replayed graph stores them without
        a history, the evaluation carries one; returns() still reads the stored values, and the stored probs are not needed then.
        -> A2CLosses(loss, policy, value, entropy, temp_entropy, rewards): the reference's fields, `loss` their sum (prepare_losses) -
        as tensors on the storage's device, not Python floats: nothing is copied to the host - and the stored rewards."""
        import torch
        from torch.distributions import Categorical
        log_probs, values, probs = (self.log_probs, self.values, self.probs) if evaluation is None else \
            (evaluation.log_probs, evaluation.values, evaluation.probs)
        rewards, adv = self.returns(final_values, discount, mode, gae_lambda)
        advantage = rewards - values
        weight = adv if mode == "gae" else advantage
        if self.use_ppo is False:
            policy_loss = torch.stack([(-log_prob * weight.detach()).mean() for log_prob in log_probs.permute(1, 0, 2)]).mean()
        else:
            policy_loss = self._ppo_loss(weight, log_probs)
        value_loss = advantage.pow(2).mean()
        if action_probs is None:
            assert probs is not None, "a2c_loss(action_probs=None) takes the stored probs (make the storage with n_probs = sum(groups)) or the evaluation's"
            action_probs = [p.contiguous() for p in torch.split(probs, list(self.groups), dim=2)]   # (the layout of the reference's stack)
        else:
            action_probs = [torch.stack([action_probs[time][a] for time in range(self.rollout_size)]) for a in range(len(action_probs[0]))]
        temp_actions = [action_prob.mean(dim=0) for action_prob in action_probs]
        batch_actions = [action_prob.mean(dim=1) for action_prob in action_probs]
        tempEntropies = torch.stack([Categorical(temp_action).entropy() for temp_action in temp_actions])
        batchEntropies = torch.stack([Categorical(batch_action).entropy() for batch_action in batch_actions])
        allEntropies = torch.stack([Categorical(action_prob).entropy() for action_prob in action_probs])
        tempEntropy = tempEntropies.mean().detach()
        batchEntropy = batchEntropies.mean()
        fullEntropy = allEntropies.mean()
        retEntropy = fullEntropy if self.use_full_entropy else batchEntropy
        policy, value, entropy, temp = policy_loss, value_coeff * value_loss, -entropy_coeff * retEntropy, entropy_coeff * tempEntropy
        loss = policy.sum() + value.sum() + entropy.sum() + temp.sum()
        return A2CLosses(loss, policy.detach(), value.detach(), entropy.detach(), temp, self.rewards.detach())


class GpuRollout(object):
    """The reference's episode_rollout (train.py:241-293) for the device layers: env a BatchedDynEnv, net a GpuFeatureExtractor, policy
    a GpuPolicyHead, storage a GpuRolloutStorage; net2, optional, a second extractor whose features are stored and fed to the policy
    beside net's (feat1).  One iteration, in the reference's order (train.py:251-278):
        feature = net(env.obs, ext, env.counts(), reset_env=the previous step's dones)
        out = policy.act(feature, out_actions=static_actions);  ext.copy_(out.next_ext)
        env.step_flat(static_actions, auto_reset=env.per_env)
        storage.insert(env.rewards, env.agent_finished(), feature, None, out.actions, out.log_probs, out.value, env.dones, probs)
    and the cursor's add_.  With graph=True (the default) the iteration is recorded ONCE, at the first collect(), with torch.cuda.graph -
    a capture fails at the first host read - and collect() replays it rollout_size times; with graph=False the same iteration runs
    eagerly.  collect() then bootstraps as train.py:284-290 does: extractor and policy.act on the last observation, insert_final of the
    features, and it returns final_value [P, 1]; net.h, net.c and policy.draw are then restored in place, so that the next rollout
    continues exactly as if no bootstrap had run.  The environment is reset by the caller before the first collect(); a lock-step
    handle (whose episode end the host decides) is stepped with auto_reset=False.  `ext` is the extractor's position input, float32
    [P, action_dim] (None for an extractor without one); `static_actions` the int32 [E, A, action_dim] tensor the step reads."""

    def __init__(self, env, net, policy, storage, net2=None, graph=True):
        import torch
        self.env, self.net, self.net2, self.policy, self.storage = env, net, net2, policy, storage
        E, A = env.num_envs, env.n_agents
        assert (storage.num_envs, storage.num_players, storage.action_cols) == (E, A, policy.action_cols)
        assert policy.n_cont == 0, "the collector steps on discrete actions"
        dev = env.device
        self.static_actions = torch.zeros((E, A, policy.action_cols), dtype=torch.int32, device=dev)
        X = getattr(net, "extended_feature_cnt", 0)
        self.ext = torch.zeros((E * A, X), dtype=torch.float32, device=dev) if X else None
        self.prev_dones = torch.zeros((E,), dtype=torch.uint8, device=dev)
        self.finished = torch.zeros((E, A), dtype=torch.bool, device=dev)
        self.use_graph = bool(graph)
        self.graph = None
        self.routes = None

    def _features(self):
        env, ce = self.env, self.env.counts()
        feats = [self.net(env.obs, self.ext, ce, reset_env=self.prev_dones)]
        if self.net2 is not None:
            feats.append(self.net2(env.obs, None, ce, reset_env=self.prev_dones))
        return feats + [None] * (2 - len(feats))

    def _iteration(self):
        env, st = self.env, self.storage
        feat0, feat1 = self._features()
        out = self.policy.act(feat0, feat1, out_actions=self.static_actions)
        if self.ext is not None:
            self.ext.copy_(out.next_ext)
        env.step_flat(self.static_actions, auto_reset=env.per_env)
        env.agent_finished(out=self.finished)
        st.insert(env.rewards, self.finished, feat0, feat1, out.actions, out.log_probs, out.value, env.dones, out.probs if st.n_probs else None)
        self.prev_dones.copy_(env.dones)
        self.routes = (self.net.last_route, self.policy.last_route, st.last_route)

    def _saved(self):
        nets = [self.net] + ([self.net2] if self.net2 is not None else [])
        for n in nets:   # (a state without a history lives in the extractor's own two tensors from here on: the ones a recording names)
            if n.h.grad_fn is None and n.c.grad_fn is None:
                n._state_into_fixed()
        return [(n, n.h, n.c, n.h.detach().clone(), n.c.detach().clone()) for n in nets], self.policy.draw.clone()

    def _restore(self, saved):
        """the extractors' state and the draw counter as they were: the same tensors, so that a recorded graph still reads and writes
        them (a tensor with a history was not written by the no_grad calls in between and is put back as it is)"""
        states, draw = saved
        for n, h0, c0, h, c in states:
            n.h, n.c = h0, c0
            if h0.grad_fn is None and c0.grad_fn is None:
                h0.copy_(h)
                c0.copy_(c)
        self.policy.draw.copy_(draw)

    def _record(self):
        """Everything of an iteration but the step runs once eagerly first - torch loads its kernels outside the recording; the step's are
        loaded with the library, by the reset - and is undone exactly; then the iteration is recorded, which runs nothing on the device."""
        import torch
        env, st = self.env, self.storage
        saved, acts, prev, fin = self._saved(), self.static_actions.clone(), self.prev_dones.clone(), self.finished.clone()
        ext = None if self.ext is None else self.ext.clone()
        kept = {k: b.clone() for k, b in st.buffers().items()}
        cur, status = st.cursor.clone(), st.status.clone()
        feat0, feat1 = self._features()
        out = self.policy.act(feat0, feat1, out_actions=self.static_actions)
        if self.ext is not None:
            self.ext.copy_(out.next_ext)
        env.agent_finished(out=self.finished)
        st.insert(env.rewards, self.finished, feat0, feat1, out.actions, out.log_probs, out.value, env.dones, out.probs if st.n_probs else None)
        self.prev_dones.copy_(env.dones)
        self._restore(saved)
        self.static_actions.copy_(acts), self.prev_dones.copy_(prev), self.finished.copy_(fin)
        if ext is not None:
            self.ext.copy_(ext)
        for k, b in st.buffers().items():
            b.copy_(kept[k])
        st.cursor.copy_(cur), st.status.copy_(status)
        torch.cuda.synchronize(env.device)
        step = getattr(env, "_episode_step", 0)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._iteration()
        env._episode_step = step   # (a lock-step handle counted the recording as a step; nothing ran)

    def collect(self):
        """rollout_size iterations, then the bootstrap -> final_value [P, 1].  A recorded iteration carries no gradient (it is recorded
        and replayed under no_grad); with graph=False the iterations run in the caller's gradient mode, as the reference's do."""
        import torch
        st = self.storage
        if self.use_graph:
            with torch.no_grad():
                if self.graph is None:
                    self._record()
                for _ in range(st.rollout_size):
                    self.graph.replay()
        else:
            for _ in range(st.rollout_size):
                self._iteration()
        with torch.no_grad():   # train.py:284-290
            saved = self._saved()
            feat0, feat1 = self._features()
            final_value = self.policy.act(feat0, feat1).value
            st.insert_final(feat0, feat1)
            self._restore(saved)
        return final_value
