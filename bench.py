#!/usr/bin/env python3
"""bench.py — throughput of the batched DynEnv step() on MI355X (contract: see the task prompt / DESIGN.md §Measurement).

A "step" = one environment step (10 fused physics substeps + Full observation + rewards) of EVERY environment of
this rank's shard = one launch of drv_step_kernel.  Workload = BASELINE.json configs[1]: DrivingEnvironment
nPlayers=10, Full obs, noise 0, 4096 envs per GPU (weak scaling over GPUs, env ids sharded by rank, one RCCL
all-gather of the packed obs|reward|done slab per step when N > 1).  Inputs (actions) are resident in HBM before
the timed region; lock-step episode resets (every 600 steps) are inside it.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--envs E] [--dump-outputs DIR] [--full [--no-cpu-baseline]]
  N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N
         or plain `python bench.py --gpus N`: without WORLD_SIZE in the environment the script starts that launcher itself, as a child

A plain run sets up, warms up, times the K steps, writes the last timed step's outputs if --dump-outputs is given and prints the
line.  --full adds everything else after the timed region: the whole-episode roofline leg, the other configurations, the batch-size
sweep, the configs[0] plumbing leg, the arranger leg, the CPU baselines, and (N > 1) the lock-step gather leg and the shard check.
"""
import argparse
import json
import os
import sys
import time

# dmabuf IPC: the pool's host driver supports nothing else, and RCCL / tensor sharing across processes fails with
# "hipIpcGetMemHandle: invalid argument" without it.  Exported by the image; kept here for a shell that dropped it (must be set
# before the HIP runtime starts, i.e. before the first torch.cuda call of this process and of every rank it starts).
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# Algorithmic HBM bytes per Driving env-step, A=10, Full obs (derivation in DESIGN.md):
# actions 20 + state read 2550 + state write 2230 + obs 10*232*4 (+8 counts) + rewards 80 + done 1
B_ALG_DRIVING_FULL_A10 = 20 + 2550 + 2230 + (9280 + 8) + 80 + 1
# RoboCup Full, A=10: actions 40 + state 3650 R + 3650 W + obs 10*5*66*4 + rewards 80 + done 1
B_ALG_ROBOCUP_FULL_A10 = 40 + 3650 + 3650 + 13200 + 80 + 1
# Driving Partial obs (configs[3]): as Full but the observation is 10 agents x 517 f32 (oracle/driving_partial.c layout)
B_ALG_DRIVING_PARTIAL_A10 = 20 + 2550 + 2230 + 10 * 517 * 4 + 80 + 1
# RoboCup Partial obs (§8 a17): as Full but the observation is 5 snapshots x 10 agents x 793 f32 (oracle/robocup_partial.h)
B_ALG_ROBOCUP_PARTIAL_A10 = 40 + 3650 + 3650 + 5 * 10 * 793 * 4 + 80 + 1
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec


def host_core_share():
    """Cores this job may use: cgroup cpu.max quota if set, else the affinity mask, capped at 16 (the per-GPU share of
    the GPU box; an un-capped 256-thread pool on a shared host measures scheduler noise, not the code)."""
    n = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()
            if q != "max":
                n = max(1, int(int(q) / int(p)))
    except (OSError, ValueError):
        pass
    if n is None:
        try:
            n = len(os.sched_getaffinity(0))
        except AttributeError:
            n = os.cpu_count() or 1
    return max(1, min(n, 16))


def cpu_baseline_oversubscribed(E, n_players, A, seed, robocup, partial, threads):
    """cpu_baseline with more OpenMP threads than the cgroup grants cores, in a CHILD process started with OMP_WAIT_POLICY=passive (idle
    workers sleep instead of spinning; libgomp reads the variable once, when it starts - the parent's own baseline keeps the default):
    256 spinning threads on a 16-core share measured 0.29 M agent-steps/s in round 5 against 6.7 M on 16, an artefact, not a rate."""
    import subprocess
    code = ("import sys, json; sys.path.insert(0, %r); import bench; "
            "print(json.dumps(bench.cpu_baseline(%d, %d, %d, %d, %r, target_seconds=8.0, partial=%r, threads=%d)))"
            % (ROOT, E, n_players, A, seed, robocup, partial, threads))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OMP_WAIT_POLICY="passive"), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600)
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
    return json.loads(lines[-1]) if r.returncode == 0 and lines else None


def cpu_baseline(E, n_players, A, seed, robocup=False, target_seconds=12.0, partial=False, threads=None):
    """The CPU restatement (oracle, kind='port') timed on this box's host cores on a bounded sample of the same
    workload.  It is a C restatement, i.e. a much stronger baseline than the reference's Python+pymunk path, which
    cannot run here (pymunk absent; the reference never ships to the GPU box)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import oracle_lib as ol
    cores = threads or host_core_share()
    ol.build()
    if robocup:
        env = ol.OracleEnv(env_type=0, num_envs=E, n_players=n_players, seed=seed, threads=cores, flags=ol.ROBOCUP_DEFAULT_FLAGS,
                           **(dict(obs_type=1, noise_type=1, noise_magnitude=3.0) if partial else {}))
    elif partial:  # ObservationType.PARTIAL = 1, NoiseType.REALISTIC = 1 (cutils.py:29-51)
        env = ol.OracleEnv(env_type=1, num_envs=E, n_players=n_players, obs_type=1, noise_type=1, noise_magnitude=3.0,
                           seed=seed, threads=cores)
    else:
        env = ol.OracleEnv(env_type=1, num_envs=E, n_players=n_players, seed=seed, threads=cores)
    env.reset()
    rng = np.random.default_rng(0)
    if robocup:
        acts = [np.stack([rng.integers(0, k, (E, A)) for k in (5, 3, 3, 7)], -1).astype(np.int32) for _ in range(8)]
    else:
        acts = [rng.integers(0, 3, size=(E, A, 2)).astype(np.int32) for _ in range(8)]
    env.step(acts[0])  # touch memory
    t0 = time.perf_counter()
    n = 0
    while True:
        env.step(acts[n % 8])
        n += 1
        dt = time.perf_counter() - t0
        if (dt >= target_seconds and n >= 5) or n >= 600:
            break
    value = E * n * A / dt
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"value": value, "unit": "agent-steps/s", "cores": cores, "kind": "port",
            "sample": "%d steps of the same %d-env %s nPlayers=%d workload (first %d steps of an episode), "
                      "oracle/liboracle.so with %d OpenMP threads, %.1f s"
                      % (n, E, ("RoboCup Partial-obs" if partial else "RoboCup") if robocup else "Driving Partial-obs" if partial else "Driving", n_players, n, cores, dt),
            "cpu_model": model}


WORKLOADS = {
    # name: (robocup, partial, players, steps per episode, B_alg, dominant kernel, BASELINE reference)
    "driving": (False, False, 10, 600, B_ALG_DRIVING_FULL_A10, "drv_step_kernel", "BASELINE.json configs[1]"),
    "robocup": (True, False, 5, 240, B_ALG_ROBOCUP_FULL_A10, "rc_step_kernel", "BASELINE.json configs[2]"),
    "driving_partial": (False, True, 10, 600, B_ALG_DRIVING_PARTIAL_A10, "drv_step_partial_kernel", "BASELINE.json configs[3]"),
    "robocup_partial": (True, True, 5, 240, B_ALG_ROBOCUP_PARTIAL_A10, "rc_step_partial_kernel", "SURVEY §8 a17; in no BASELINE config"),
}


def spread_positions(n, episode_len):
    """positions inside one episode of the n timed steps that do not fill a whole episode: stratified, step j in the middle of the
    j-th of n equal slices (so that the sample weighs the cheap start and the expensive end of an episode like the episode does)"""
    return [min(episode_len - 1, int((j + 0.5) * episode_len / n)) for j in range(n)]


def spread_blocks(n, episode_len, max_blocks=4):
    """N > 1: the same n steps as up to `max_blocks` contiguous blocks (the pipelined transport overlaps inside a block), centred in
    equal slices of the episode -> [(first step, number of steps)]"""
    nb = min(max_blocks, n)
    sizes = [n // nb + (1 if b < n % nb else 0) for b in range(nb)]
    return [(max(0, min(episode_len - sizes[b], int((b + 0.5) * episode_len / nb) - sizes[b] // 2)), sizes[b]) for b in range(nb)]


def kernel_source_sha():
    """sha256 over the kernel sources the shipped library is built from (dynenv_amd/csrc/* + include/*), first 16 hex digits:
    stamps profiles/pmc_traffic.json, so that a traffic figure measured on other kernels is never reported for these."""
    import hashlib
    h = hashlib.sha256()
    for d in (os.path.join(ROOT, "dynenv_amd", "csrc"), os.path.join(ROOT, "include")):
        for name in sorted(os.listdir(d)):
            if name.endswith((".hip", ".h")):
                with open(os.path.join(d, name), "rb") as f:
                    h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def measured_traffic(kernel):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 FETCH_SIZE / WRITE_SIZE passes (profiles/pmc_traffic.json,
    written by tools/profile_round.sh on the GPU box; FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950).  A PMC
    pass cannot run inside this process, so the file is stamped with the hash of the kernel sources it was measured on: if
    the sources have changed since, the figure is stale and null is reported.  -> (bytes or None, detail dict)"""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            t = json.load(f)
    except (OSError, ValueError):
        return None, {"traffic_source": None}
    sha = kernel_source_sha()
    if t.get("kernel_source_sha16") != sha:
        return None, {"traffic_source": "profiles/pmc_traffic.json is STALE (measured on kernel sources %s, these are %s): null"
                                        % (t.get("kernel_source_sha16"), sha)}
    d = t.get(kernel + "_detail", {})
    return t.get(kernel + "_bytes_per_launch"), {"traffic_source": "profiles/pmc_traffic.json (kernel sources %s)" % sha,
                                                 "traffic_whole_step": d.get("step_bytes_all_kernels")}


def measured_sq(kernel):
    """What actually bounds these kernels (issue and latency, not bytes): the SQ counters of `kernel` from the committed
    rocprofv3 --pmc passes (profiles/sq_counters.json, tools/profile_round.sh), stamped with the kernel-source hash like the traffic
    figures: stale -> nulls.  -> dict(valu_busy, wave_time_shares, insts_per_wave, sq_source)"""
    try:
        with open(os.path.join(ROOT, "profiles", "sq_counters.json")) as f:
            t = json.load(f)
    except (OSError, ValueError):
        return {"valu_busy": None, "wave_time_shares": None, "sq_source": None}
    sha = kernel_source_sha()
    if t.get("kernel_source_sha16") != sha:
        return {"valu_busy": None, "wave_time_shares": None,
                "sq_source": "profiles/sq_counters.json is STALE (measured on kernel sources %s, these are %s): null" % (t.get("kernel_source_sha16"), sha)}
    d = t.get(kernel)
    if not d:
        return {"valu_busy": None, "wave_time_shares": None, "sq_source": "profiles/sq_counters.json holds no %s" % kernel}
    return {"valu_busy": d["valu_busy"], "wave_time_shares": d["wave_time_shares"], "insts_per_wave": d.get("insts_per_wave"),
            "valu_busy_is": "SQ_INSTS_VALU x 4 cycles / (1024 SIMDs x the launch's duration x 2.4 GHz): the share of the chip's VALU issue "
                            "slots the launch used - a LOWER bound on VALU-busy time (an fp64 instruction holds its SIMD longer than 4 cycles)",
            "sq_source": "profiles/sq_counters.json (kernel sources %s, launch %.1f us under the profiler)" % (sha, d.get("launch_us", float("nan")))}


def episode_leg(torch, device, workload, E, seed, n_players=None, env_id_offset=0, no_isolation=False):
    """One whole episode of `workload` (every step of it, the lock-step reset excluded), timed with HIP events on the launch
    stream: the episode mean is what a training run sees - a window at the start of an episode flatters Driving, whose
    contact work grows over the episode."""
    from dynenv_amd import BatchedDynEnv, DynEnvType, NoiseType, ObservationType
    robocup, partial, players, ep_steps, b_alg, kernel, ref = WORKLOADS[workload]
    players = n_players if n_players is not None else players
    A = 2 * players if robocup else players
    kw = dict(observationType=ObservationType.PARTIAL, noiseType=NoiseType.REALISTIC, noiseMagnitude=3) if partial else {}
    g = torch.Generator(device=device).manual_seed(4321)
    if robocup:
        hi = torch.tensor([5, 3, 3, 7], device=device)
        pool = [(torch.rand((E, A, 4), generator=g, device=device) * hi).to(torch.int32) for _ in range(16)]
    else:
        pool = [torch.randint(0, 3, (E, A, 2), generator=g, device=device, dtype=torch.int32) for _ in range(16)]

    def fresh_env():  # both passes below run the SAME episode (episode index 2 of a fresh handle: identical trajectories)
        if no_isolation:  # read by dynenv_create: the plain grid, no SIMD isolation of the slow environments
            os.environ["DYNENV_NO_ISOLATION"] = "1"
        try:
            return fresh_env_()
        finally:
            if no_isolation:
                del os.environ["DYNENV_NO_ISOLATION"]

    def fresh_env_():
        env = BatchedDynEnv(DynEnvType.ROBO_CUP if robocup else DynEnvType.DRIVE, E, players, seed=seed, device=device,
                            env_id_offset=env_id_offset, **kw)
        env.reset_flat()
        for i in range(3):  # untimed: first-touch of the buffers, then a fresh episode
            env.step_flat(pool[i & 15], auto_reset=False)
        env.reset_flat()
        torch.cuda.synchronize(device)
        return env
    env = fresh_env()
    k0, k1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    k0.record()
    for i in range(ep_steps):
        env.step_flat(pool[i & 15], auto_reset=False)
    k1.record()
    torch.cuda.synchronize(device)
    ms = k0.elapsed_time(k1) / ep_steps
    assert env.error_flags() == 0
    env.close()
    if no_isolation:  # only the back-to-back figure is wanted
        return {"workload": workload, "envs": E, "steps": ep_steps, "ms_per_step": ms, "value": E * A / (ms * 1e-3), "unit": "agent-steps/s"}
    env = fresh_env()
    # the named kernel's OWN launch duration: a second pass over the same episode (same seed, same actions) with the library
    # recording HIP events on the launch stream right before and after that kernel (dynenv_set_step_events), a fresh event
    # set per step and no host wait in between, so the launches stay back to back as in the pass above and the Partial
    # paths' trailing kernels are not counted.  An interval between two events contains one event record (a barrier packet,
    # ~5 us here): its cost is measured by a fourth event recorded right behind the third and subtracted
    import ctypes as C
    evs = [tuple(torch.cuda.Event(enable_timing=True) for _ in range(4)) for _ in range(ep_steps)]
    for tr in evs:
        for ev in tr:
            ev.record()  # creates the hipEvent_t
    torch.cuda.synchronize(device)
    for i in range(ep_steps):
        eb, em, ee, ex = evs[i]
        env._lib.dynenv_set_step_events(env._h, C.c_void_p(eb.cuda_event), C.c_void_p(em.cuda_event), C.c_void_p(ee.cuda_event))
        env.step_flat(pool[i & 15], auto_reset=False)
        ex.record()  # nothing between `ee` and `ex`: their distance is what an event record itself costs on this stream
    env._lib.dynenv_set_step_events(env._h, None, None, None)
    torch.cuda.synchronize(device)
    ev_cost = sum(ee.elapsed_time(ex) for eb, em, ee, ex in evs) / ep_steps
    kern_ms = sum(eb.elapsed_time(em) for eb, em, ee, ex in evs) / ep_steps - ev_cost
    step_ms = sum(eb.elapsed_time(ee) for eb, em, ee, ex in evs) / ep_steps - ev_cost
    err = env.error_flags()
    iso = None
    if not robocup:  # Driving: did the library isolate its slow environments on SIMDs of their own (scheduling only)?
        dc = env.debug_counters()
        iso = {"on": dc["isolated_next"] >= 0, "mode": int(dc["isolation_mode"]), "isolated_in_last_step": max(int(dc["isolated_next"]), 0),
               "placeholder_timeouts": int(dc["isolation_timeouts"]), "placement_validated": int(dc["placement_validated"]),
               "launches_whose_placement_did_not_validate": int(dc["placement_invalid_launches"])}
    env.close()
    out = {"workload": workload, "reference": ref, "envs": E, "n_agents": A, "steps": ep_steps, "ms_per_step": ms,
           "value": E * A / (ms * 1e-3), "unit": "agent-steps/s", "kernel_error_flags": err}
    if A == 10:
        # the algorithmic bytes are those of the WHOLE step: where a step is more than one launch (Partial observations: the
        # deferred / finalize kernels do part of the work) they are divided by the time of all of its kernels
        basis_ms = step_ms if partial else kern_ms
        achieved = b_alg * E / (basis_ms * 1e-3) / 1e9
        traffic, tdetail = measured_traffic(kernel)
        if partial and tdetail.get("traffic_whole_step") is not None:
            traffic = tdetail["traffic_whole_step"]
        out["roofline"] = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                           "traffic": traffic, "kernel": kernel, "launch_ms": kern_ms, "step_ms_all_kernels": step_ms,
                           "achieved_over": "step_ms_all_kernels" if partial else "launch_ms",
                           "step_ms_back_to_back": ms, "event_record_cost_ms": ev_cost, "alg_bytes_per_env_step": b_alg,
                           "env_steps_per_launch": E}
        out["roofline"].update(tdetail)
        out["roofline"].update(measured_sq(kernel))   # `frac` stays the HBM figure; valu_busy / wave_time_shares say what binds instead
    if iso is not None:
        out["simd_isolation"] = iso
    return out


def batch_leg(torch, device, E, K, seed, steps=600):
    """Throughput against batch size / sub-batches (never the headline): Driving nPlayers=10 Full over one whole episode with
    E environments as K handles of E / K (env_id_offset = k E / K: the same global environments, results identical to one
    handle - tools/split_batch_probe.py checks the digests) on K streams, stepped round-robin.  A launch lasts as long as its
    slowest environment and 4096 environments are exactly one residency round of the chip (16 waves per CU), so a bigger
    batch backfills the tail of a launch with later blocks; K > 1 overlaps the tails of the sub-batches."""
    from dynenv_amd import BatchedDynEnv, DynEnvType
    A, D, n = 10, 232, E // K
    obs = torch.zeros((E, 1, A, D), dtype=torch.float32, device=device)
    rew = torch.zeros((E, A), dtype=torch.float64, device=device)
    don = torch.zeros((E,), dtype=torch.uint8, device=device)
    envs = [BatchedDynEnv(DynEnvType.DRIVE, n, 10, seed=seed, device=device, env_id_offset=k * n,
                          out_buffers=(obs[k * n:(k + 1) * n], rew[k * n:(k + 1) * n], don[k * n:(k + 1) * n])) for k in range(K)]
    streams = [torch.cuda.Stream(device=device) for _ in range(K)] if K > 1 else [torch.cuda.current_stream(device)]
    g = torch.Generator(device=device).manual_seed(4321)
    pool = [torch.randint(0, 3, (E, A, 2), generator=g, device=device, dtype=torch.int32) for _ in range(16)]
    sub = [[p[k * n:(k + 1) * n] for k in range(K)] for p in pool]

    def episode():
        for k in range(K):
            with torch.cuda.stream(streams[k]):
                envs[k].reset_flat()
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for i in range(steps):
            for k in range(K):
                with torch.cuda.stream(streams[k]):
                    envs[k].step_flat(sub[i & 15][k], auto_reset=False)
        torch.cuda.synchronize(device)
        return time.perf_counter() - t0
    episode()
    dt = episode()
    for e in envs:
        e.close()
    del obs, rew, don, pool, sub
    return {"envs": E, "handles_on_streams": K, "steps": steps, "ms_per_step": dt / steps * 1e3, "value": E * A * steps / dt,
            "unit": "agent-steps/s"}


def plumbing_leg(torch, device, seed):
    """BASELINE.json configs[0] / BASELINE.md B0: DrivingEnvironment nPlayers=2, Full obs, noise 0, ONE environment - on the GPU
    (one wave) and on one host thread through the oracle, one whole episode each."""
    gpu = episode_leg(torch, device, "driving", 1, seed, n_players=2)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import oracle_lib as ol
    from dynenv_amd import BatchedDynEnv, DynEnvType
    ol.build()
    env = ol.OracleEnv(env_type=1, num_envs=1, n_players=2, seed=seed, threads=1)
    env.reset()
    rng = np.random.default_rng(0)
    acts = rng.integers(0, 3, size=(600, 1, 2, 2)).astype(np.int32)
    t0 = time.perf_counter()
    for a in acts:
        env.step(a)
    dt = time.perf_counter() - t0
    # BASELINE.md B0 asks for the parity result of this configuration beside its rate: the same 600 steps on both sides, untimed,
    # observations / rewards / dones of every step compared bit for bit (the oracle here is the CHECKER, never the thing measured)
    genv = BatchedDynEnv(DynEnvType.DRIVE, 1, 2, seed=seed, device=device)
    oenv = ol.OracleEnv(env_type=1, num_envs=1, n_players=2, seed=seed, threads=1)
    same = bool(np.array_equal(genv.reset_flat().cpu().numpy(), oenv.reset()))
    mismatches = 0 if same else 1
    for a in acts:
        og, rg, dg = genv.step_flat(a, auto_reset=False)
        oc, rc, dc = oenv.step(a)
        ok = np.array_equal(og.cpu().numpy(), oc) and np.array_equal(rg.cpu().numpy(), rc) and np.array_equal(dg.cpu().numpy(), dc)
        mismatches += 0 if ok else 1
    parity = {"steps_compared": len(acts), "steps_with_a_mismatch": mismatches, "error_flags": genv.error_flags(),
              "what": "reset observation + observations, rewards, dones of all 600 steps of the episode, HIP path vs CPU oracle, bit for bit"}
    genv.close()
    return {"workload": "DrivingEnvironment nPlayers=2 Full obs, noise=0, 1 env (BASELINE.json configs[0])", "steps": 600, "parity": parity,
            "gpu_env_steps_per_s": 1.0 / (gpu["ms_per_step"] * 1e-3), "gpu_ms_per_step": gpu["ms_per_step"],
            "cpu_port_env_steps_per_s": 600 / dt, "cpu_threads": 1,
            "note": "one environment cannot fill a GPU (one wave of 64 lanes): this leg is the plumbing check BASELINE.md asks for"}


def arranger_leg(torch, device, E, seed, feat=128, reps=30):
    """SURVEY section 8 f1, the HBM-bound part of the path: the GPU arranger on real Driving Full observations of E environments -
    rearrange_inputs (ragged -> per-type rows) and rearrange_outputs (embeddings of width `feat` -> the padded [T, maxCount, P, F]
    tensor, written once).  Algorithmic bytes as tools/bench_arranger.py counts them; peak 8 TB/s."""
    from dynenv_amd import BatchedDynEnv, DynEnvType, GpuInOutArranger, groups_for
    env = BatchedDynEnv(DynEnvType.DRIVE, E, 10, seed=seed, device=device)
    env.reset_flat()
    g = torch.Generator(device=device).manual_seed(1)
    for _ in range(20):
        obs, _, _ = env.step_flat(torch.randint(0, 3, (E, env.n_agents, 2), generator=g, device=device, dtype=torch.int32), auto_reset=False)
    obs = obs.contiguous()
    cnt = env.counts()
    types = groups_for(env)["movable"]
    arr = GpuInOutArranger(types, E, env.n_agents, env.n_time_steps, env.obs_dim)
    inputs, countArr = arr.rearrange_inputs(obs, cnt)
    outs = [torch.randn((i.shape[0], feat), device=device) for i in inputs]
    padded, _ = arr.rearrange_outputs(outs, countArr)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    for _ in range(reps):
        arr.rearrange_inputs(obs, cnt)
    ev[1].record()
    for _ in range(reps):
        padded, _ = arr.rearrange_outputs(outs, countArr)
    ev[2].record()
    torch.cuda.synchronize()
    ms_in, ms_out = ev[0].elapsed_time(ev[1]) / reps, ev[1].elapsed_time(ev[2]) / reps
    n_obj = [int(i.shape[0]) for i in inputs]
    b_out = sum(n_obj) * feat * 4 + padded.numel() * 4
    env.close()
    traffic, tdetail = measured_traffic("arr_pad_cols_kernel")   # (tools/profile_round.sh "hbm": the same sizes under rocprofv3 --pmc; stale -> null)
    return {"what": "GpuInOutArranger on Driving Full observations (SURVEY 8 f1)", "envs": E, "objects": n_obj, "max_count": int(countArr[1]),
            "embed_width": feat, "rearrange_inputs_ms": ms_in, "rearrange_outputs_ms": ms_out,
            "roofline": {"bound": "hbm", "kernel": "arr_pad_cols_kernel", "alg_bytes": b_out, "achieved": b_out / (ms_out * 1e-3) / 1e9,
                         "peak": 8000.0, "unit": "GB/s", "frac": b_out / (ms_out * 1e-3) / 1e9 / 8000.0, "traffic": traffic,
                         "traffic_source": tdetail.get("traffic_source")}}


DUMP_BUDGET_BYTES = 64 * 10 ** 6


def dump_outputs(torch, dirname, env, env_id_offset, budget=DUMP_BUDGET_BYTES):
    """What the last step_flat() call handed its caller - obs [E, T, A, D] float32, rewards [E, A] float64, dones [E] (uint8, written
    as float32), and terminal_obs when that step ended the episode (auto-reset: obs is then the reset observation) - as DIR/<name>.npy,
    plus env_ids.npy (float64), the global environment ids of the rows written.  All environments while they fit in `budget` bytes,
    else a fixed sample (numpy default_rng(0), sorted): the files of two runs with the same arguments are comparable row for row."""
    import numpy as np
    outs = {"obs": env.obs, "rewards": env.rewards, "dones": env.dones}
    if getattr(env, "last_done", False) and env.terminal_obs is not None:
        outs["terminal_obs"] = env.terminal_obs
    E = env.num_envs
    per_env = 8 + sum(t[0].numel() * (8 if t.dtype == torch.float64 else 4) for t in outs.values())
    k = min(E, (budget - 4096 * (len(outs) + 1)) // per_env)   # (4 KB per file for the .npy headers)
    ids = np.arange(E) if k == E else np.sort(np.random.default_rng(0).choice(E, size=k, replace=False))
    sel = torch.from_numpy(ids).to(env.obs.device)
    os.makedirs(dirname, exist_ok=True)
    for name, t in outs.items():
        a = t.index_select(0, sel).cpu().numpy()
        np.save(os.path.join(dirname, name + ".npy"), a if a.dtype == np.float64 else a.astype(np.float32))
    np.save(os.path.join(dirname, "env_ids.npy"), (ids + env_id_offset).astype(np.float64))
    return {"dir": dirname, "files": sorted(list(outs) + ["env_ids"]), "envs_written": int(k), "envs": E}


def launch_ranks(n):
    """Start `python -m torch.distributed.run --nnodes=1 --nproc-per-node n --master-addr 127.0.0.1 --master-port P bench.py
    <the same arguments>` as a child process; -> its return code.  stdout of the job is rank 0's one JSON line (every rank diverts
    whatever else would land on stdout to stderr); stderr passes through."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    r = subprocess.run(cmd, stdout=subprocess.PIPE)
    lines = [ln for ln in r.stdout.decode(errors="replace").splitlines() if ln.strip()]
    json_lines = [ln for ln in lines if ln.lstrip().startswith("{")]
    for ln in lines:
        if ln not in json_lines:
            print(ln, file=sys.stderr)
    if json_lines:
        print(json_lines[-1], flush=True)
    if r.returncode == 0 and len(json_lines) != 1:
        print("bench.py: expected one JSON line from rank 0, got %d" % len(json_lines), file=sys.stderr)
        return 1
    return r.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default: 2 whole episodes of the workload)")
    ap.add_argument("--warmup", type=int, default=None, help="warm-up steps (default: 1 whole episode of the workload)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the outputs of the last timed step as DIR/<name>.npy (float32 / float64, "
                         "at most 64 MB: a fixed sample of the environments where all of them would not fit)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the roofline, other-configuration, batch-size, plumbing, arranger and "
                         "CPU-baseline legs (N > 1: the lock-step gather leg and the shard check)")
    ap.add_argument("--envs", type=int, default=4096, help="environments per GPU")
    ap.add_argument("--players", type=int, default=None)
    ap.add_argument("--workload", choices=["driving", "robocup", "driving_partial", "robocup_partial"], default="driving",
                    help="driving = BASELINE configs[1] (the headline metric); robocup = configs[2]; driving_partial = "
                         "configs[3] (Partial obs + Realistic noise magnitude 3); the latter two are reported on request")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--no-extra-legs", action="store_true",
                    help="with --full: skip the other BASELINE configurations, the batch-size, plumbing and arranger legs (N = 1 only)")
    ap.add_argument("--roofline-only", action="store_true",
                    help="profiling runs (tools/profile_round.sh; implies --full): skip the warm-up and the timed window and run only the "
                         "whole-episode roofline leg, so that every launch a profiler sees belongs to it; the line says so in `mode`")
    ap.add_argument("--no-gather", action="store_true", help="skip the end-of-step all-gather (data-parallel consumer)")
    ap.add_argument("--force-gather", action="store_true",
                    help="rehearsal on a one-GPU box: run the N > 1 code path (slab, pack, all-gather, unpack) with world_size 1")
    ap.add_argument("--transport", choices=("compact", "tail", "dense"), default="compact",
                    help="N > 1: form in which observations cross xGMI (compact = the most compact exact form of the layout)")
    ap.add_argument("--ring", type=int, default=4, help="N > 1: slabs in flight (the host runs at most this many steps ahead of the transports)")
    ap.add_argument("--sync-gather", action="store_true",
                    help="N > 1: wait for the all-gather of step k before launching step k+1 (lock-step consumer); by default "
                         "the transport of step k runs on a side stream beside the following kernels (ring of --ring slabs)")
    ap.add_argument("--rehearse-one-gpu", action="store_true",
                    help="rehearsal of an N > 1 launch on a box with ONE GPU: every rank uses cuda:0 and the process group is gloo "
                         "(RCCL refuses two ranks on one device); slabs, pack / unpack kernels, side stream and ring are the real ones. "
                         "The line it prints says so in config.parallelism and is not a measurement")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python3 bench.py --gpus N` typed as is: this process - which has not imported torch or touched the GPU - starts the
        # one-process-per-GPU job as a CHILD (never an exec), relays rank 0's single JSON line and exits with the child's code
        sys.exit(launch_ranks(args.gpus))

    # stdout carries exactly one JSON line: anything libraries print meanwhile (RCCL's version banner at init, ...) is
    # diverted to stderr at the file-descriptor level until the result is printed
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    import torch
    from dynenv_amd import BatchedDynEnv, DynEnvType
    from dynenv_amd.distributed import PackedSlab, StepGather

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch N>1 through torch.distributed.run (one process per GPU)")
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    if args.rehearse_one_gpu:
        local_rank = 0
    ndev = torch.cuda.device_count()
    if ndev > 0 and local_rank >= ndev:  # a launcher that shows each rank only its own GPU (ROCR/HIP_VISIBLE_DEVICES)
        local_rank %= ndev
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or args.force_gather:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if args.rehearse_one_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)

    robocup = args.workload in ("robocup", "robocup_partial")
    partial = args.workload in ("driving_partial", "robocup_partial")
    n_players = args.players if args.players is not None else (5 if robocup else 10)
    env_type = DynEnvType.ROBO_CUP if robocup else DynEnvType.DRIVE
    E = args.envs
    A = 2 * n_players if robocup else n_players
    if args.steps is None:
        args.steps = 2 * WORKLOADS[args.workload][3]
    if args.warmup is None:
        args.warmup = WORKLOADS[args.workload][3]
    slab = gather = None
    out_buffers = None
    obs_kw = {}
    if partial:
        from dynenv_amd import ObservationType, NoiseType
        obs_kw = dict(observationType=ObservationType.PARTIAL, noiseType=NoiseType.REALISTIC, noiseMagnitude=3)
    if (world > 1 or args.force_gather) and not args.no_gather:
        probe = BatchedDynEnv(env_type, 1, n_players, device=device, **obs_kw)
        T, D = probe.n_time_steps, probe.obs_dim
        from dynenv_amd.distributed import transport_layout, shared_tail_split
        # Driving Full: self blocks + the shared tail travel once per env (exact; 250 instead of 2320 floats for 10 agents)
        layout = {} if args.transport == "dense" else dict(split=shared_tail_split(probe)) if args.transport == "tail" else transport_layout(probe)
        probe.close()
        slab = PackedSlab(torch, device, E, T, A, D, **layout)
        more = [] if args.sync_gather else [PackedSlab(torch, device, E, T, A, D, **layout) for _ in range(args.ring - 1)]
        out_buffers = (slab.obs, slab.rewards, slab.dones)
        gather = StepGather(torch, dist, slab, more=more)
    env = BatchedDynEnv(env_type, E, n_players, seed=args.seed, device=device, env_id_offset=rank * E,
                        out_buffers=out_buffers, **obs_kw)
    preflight = None
    if dist is not None:
        # Before anything is timed, every rank says where it is and what it owns, so that the first real multi-GPU record explains
        # itself if it fails: world size and backend as torch.distributed sees them, the device this rank bound, its slice of the
        # global environment ids, the bytes of the slab it contributes to every all-gather.
        props = torch.cuda.get_device_properties(device)
        mine = {"rank": rank, "world_size": dist.get_world_size(), "backend": dist.get_backend(), "local_rank": local_rank,
                "device": "cuda:%d %s (%d CUs, %.0f GB)" % (local_rank, props.name, props.multi_processor_count, props.total_memory / 2 ** 30),
                "visible_devices": ndev, "env_ids": [rank * E, (rank + 1) * E], "slab_bytes": (None if slab is None else slab.nbytes),
                "transport": (None if gather is None else args.transport), "pid": os.getpid()}
        print("[bench preflight] rank %(rank)d of world_size %(world_size)d (%(backend)s): %(device)s, %(visible_devices)d visible; environments "
              "[%(env_ids)s); slab %(slab_bytes)s B (%(transport)s)" % dict(mine, env_ids="%d, %d" % tuple(mine["env_ids"])), file=sys.stderr, flush=True)
        preflight = [None] * world
        dist.all_gather_object(preflight, mine)
    # synthetic inputs: i.i.d. uniform actions (action_space MultiDiscrete([3,3])), resident in HBM
    g = torch.Generator(device=device).manual_seed(1234 + rank)
    if robocup:  # MultiDiscrete([5, 3, 3, 7]) RoboCupEnvironment.py:342
        hi = torch.tensor([5, 3, 3, 7], device=device)
        pool = [(torch.rand((E, A, 4), generator=g, device=device) * hi).to(torch.int32) for _ in range(64)]
    else:
        pool = [torch.randint(0, 3, (E, A, 2), generator=g, device=device, dtype=torch.int32) for _ in range(64)]

    step_no = [0]

    def one_step(i):
        if gather is None:
            env.step_flat(pool[i & 63])
        elif args.sync_gather:
            env.step_flat(pool[i & 63])
            gather()
        else:  # all-gather of step k overlaps the kernel of step k+1; a slab is rewritten only after its gather was waited for
            k = step_no[0]
            step_no[0] += 1
            gather.release(k)
            sl = gather.slabs[k % len(gather.slabs)]
            env.use_buffers(sl.obs, sl.rewards, sl.dones)
            env.step_flat(pool[i & 63])
            gather.start(k)

    if args.roofline_only:
        args.steps, args.warmup, args.no_extra_legs, args.no_cpu_baseline, args.full = 0, 0, True, True, True
    if args.dump_outputs and args.steps <= 0:
        raise SystemExit("bench.py: --dump-outputs needs at least one timed step")
    env.reset_flat()
    for i in range(args.warmup):
        one_step(i)

    def fence():
        if gather is not None and not args.sync_gather:
            gather.drain()
        torch.cuda.synchronize(device)
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(device)

    # ---- the timed region: EXACTLY args.steps steps, chosen so that they weigh an episode the way a training run does.
    # A Driving step costs 0.10 ms at the start of an episode and 0.25 ms at its end (contacts accumulate), so K consecutive
    # steps right after the warm-up measure the cheap end only.  Instead: K // L whole episodes run back to back (L = steps per
    # episode; lock-step resets inside the timed region), and the remaining K % L steps are spread EVENLY over one
    # further episode (stratified sample: timed step j sits at position (j + 1/2) L / (K % L)), the steps between them advance
    # the same handle untimed.  N = 1: every timed step is bracketed by HIP events on the launch stream (nothing subtracted:
    # the interval holds the kernel(s) and one event record).  N > 1: the spread steps are grouped into a few contiguous blocks,
    # each bracketed by barrier + synchronize on both sides (the pipelined transport overlaps inside a block).
    L_ep = WORKLOADS[args.workload][3]
    n_full, n_spread = divmod(args.steps, L_ep)
    if args.roofline_only:  # no timed region at all: every launch of the process belongs to the whole-episode leg
        n_full = n_spread = 0
    pos = [0]  # position inside the current episode (auto-reset at L_ep)

    def advance(n):  # (the handle resets itself every L_ep steps: pos follows its position inside the episode)
        for _ in range(n):
            one_step(pos[0])
            pos[0] = (pos[0] + 1) % L_ep
    pos[0] = args.warmup % L_ep
    untimed_advance = 0
    elapsed, gpu_ms, timed_at = 0.0, 0.0, []
    raw_extra_ms = [0.0]  # what was subtracted from the timed region (N = 1 spread steps: one event record per step)
    fence()
    if n_full:
        if pos[0]:  # start whole episodes at an episode boundary
            untimed_advance += L_ep - pos[0]
            advance(L_ep - pos[0])
            fence()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        ev0.record()
        advance(n_full * L_ep)
        ev1.record()
        fence()
        elapsed += time.perf_counter() - t0
        gpu_ms += ev0.elapsed_time(ev1)
        timed_at.append("%d whole episode(s) of %d steps, back to back, resets included" % (n_full, L_ep))
    if n_spread:
        if pos[0]:
            untimed_advance += L_ep - pos[0]
            advance(L_ep - pos[0])
        at = spread_positions(n_spread, L_ep)
        if dist is None:
            # an interval between two events holds the step's kernel(s) and ONE event record (a barrier packet, ~5 us on this stream),
            # which a step in a run of steps does not contain: a third event right behind the second measures what a record costs.
            # NOTHING is subtracted from `value` (round 6; VERDICT r5: "the headline still subtracts ..."): the record stays in the
            # timed region, which makes the figure conservative; the corrected one is reported beside it (ms_per_step_minus_event_record)
            evs = [tuple(torch.cuda.Event(enable_timing=True) for _ in range(3)) for _ in at]
            fence()
            for j, p_ in enumerate(at):
                untimed_advance += p_ - pos[0]
                advance(p_ - pos[0])
                evs[j][0].record()
                advance(1)
                evs[j][1].record()
                evs[j][2].record()
            fence()
            ev_cost_ms = sum(b.elapsed_time(c) for a, b, c in evs)
            raw_extra_ms[0] = ev_cost_ms
            dt_ms = sum(a.elapsed_time(b) for a, b, c in evs)
            elapsed += dt_ms * 1e-3
            gpu_ms += dt_ms
            timed_at.append("%d single steps at positions %s of one episode, HIP events around each (each interval includes the one event record "
                            "that closes it, %.1f us: not subtracted)" % (n_spread, at, ev_cost_ms / n_spread * 1e3))
        else:
            blocks = spread_blocks(n_spread, L_ep)
            n_blocks, starts, sizes = len(blocks), [b_[0] for b_ in blocks], [b_[1] for b_ in blocks]
            for b in range(n_blocks):
                untimed_advance += starts[b] - pos[0]
                advance(starts[b] - pos[0])
                fence()
                eb0, eb1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                eb0.record()
                advance(sizes[b])
                eb1.record()
                fence()
                elapsed += time.perf_counter() - t0
                gpu_ms += eb0.elapsed_time(eb1)
            timed_at.append("%d steps as %d blocks %s of one episode, barrier + synchronize around each block"
                            % (n_spread, n_blocks, [(a, a + n - 1) for a, n in zip(starts, sizes)]))
    # the last step above was the last timed one: its buffers still hold what it returned
    dumped = dump_outputs(torch, args.dump_outputs, env, rank * E) if args.dump_outputs and rank == 0 else None
    per_rank = None
    if dist is not None:
        # every rank's own wall clock and GPU time of the timed region: the line is self-checking (value uses the MAX)
        mine = torch.tensor([elapsed, gpu_ms / max(args.steps, 1)], dtype=torch.float64, device=device)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [[float(x[0]), float(x[1])] for x in allr]
        elapsed = max(x[0] for x in per_rank)
    err = env.error_flags()

    # the lock-step variant in the same line (N > 1): the global view of step k is awaited before step k + 1 is launched
    sync_leg = None
    if args.full and gather is not None and not args.sync_gather:
        n_sync = min(args.steps, 100)
        env.use_buffers(slab.obs, slab.rewards, slab.dones)
        for i in range(3):
            env.step_flat(pool[i & 63])
            gather()
        fence()
        ts = time.perf_counter()
        for i in range(n_sync):
            env.step_flat(pool[i & 63])
            gather()
        fence()
        dt = time.perf_counter() - ts
        if dist is not None:
            t = torch.tensor([dt], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        sync_leg = {"steps": n_sync, "ms_per_step": dt / n_sync * 1e3, "value": E * world * n_sync * A / dt,
                    "note": "--sync-gather semantics: all-gather of step k completed before step k + 1 is launched"}

    # roofline leg: the dominant kernel over one WHOLE episode (no reset, no collective), HIP events on the launch stream.
    # N > 1: every rank runs it on its own shard's environment ids (kernel alone, no transport), so that a SCALE record can be
    # cross-checked against the N = 1 BENCH record rank by rank without trusting the timed window
    roofline = None
    full = None
    ep_steps = WORKLOADS[args.workload][3]
    shard_check = None
    if args.full and (rank == 0 or dist is not None):
        full = episode_leg(torch, device, args.workload, E, args.seed, n_players=n_players, env_id_offset=rank * E)
        roofline = full.get("roofline")
    if args.full and dist is not None:
        mine = torch.tensor([float(env.cfg.env_id_offset), full["value"], full["ms_per_step"], float(env.num_envs)], dtype=torch.float64, device=device)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        offs = [int(x[0]) for x in allr]
        shard_check = {"rccl_world_size": dist.get_world_size(), "backend": dist.get_backend(), "n_gpus_flag": args.gpus,
                       "env_id_offset_per_rank": offs, "envs_per_rank": [int(x[3]) for x in allr],
                       "value_full_episode_per_rank": [float(x[1]) for x in allr],
                       "ms_per_step_full_episode_per_rank": [float(x[2]) for x in allr], "preflight": preflight,
                       "note": "per rank: the N = 1-equivalent whole-episode figure of that rank's shard (kernel alone, no transport)"}
        # a line that claims N GPUs must have been produced by N RCCL ranks, each owning its own slice of the global environment ids
        assert dist.get_world_size() == args.gpus or args.force_gather, "bench.py --gpus %d ran with world size %d" % (args.gpus, dist.get_world_size())
        assert offs == [r * E for r in range(world)], "environment id offsets %s are not rank * %d" % (offs, E)

    if rank == 0:
        env_steps = E * world * args.steps
        value = env_steps * A / elapsed if elapsed > 0 else None
        what = ("RoboCupEnvironment nPlayers=%d %s, 50 substeps/step" % (n_players, "Partial obs + Realistic noise magnitude 3" if partial else "Full obs")
                if robocup else
                "DrivingEnvironment nPlayers=%d %s, 10 substeps/step" % (A, "Partial obs + Realistic noise magnitude 3" if partial else "Full obs, noise=0"))
        workload_text = ("%s, %d envs per GPU (%s), lock-step resets every %d steps; timed after %d warm-up steps: %s"
                         % (what, E, WORKLOADS[args.workload][6], ep_steps, args.warmup, "; ".join(timed_at)))
        out = {
            "metric": "agent-steps/s", "value": value, "unit": "agent-steps/s", "n_gpus": world,
            **({"mode": "roofline-only: no timed region (value null); read roofline / ms_per_step_full_episode"} if args.roofline_only else {}),
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": (elapsed / args.steps * 1e3 if elapsed > 0 else None),
            "ms_per_step_raw": (elapsed / args.steps * 1e3 if elapsed > 0 else None),
            "value_raw": (env_steps * A / elapsed if elapsed > 0 else None),
            "ms_per_step_minus_event_record": ((elapsed * 1e3 - raw_extra_ms[0]) / args.steps if elapsed > 0 and raw_extra_ms[0] else None),
            "raw_is": "= value / ms_per_step since round 6: the timed region with NOTHING subtracted (N = 1: each spread step's interval still holds the one HIP event record that brackets it)",
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": workload_text,
                       "envs_per_gpu": E, "n_players": n_players, "n_agents": A, "obs": "partial" if partial else "full", "gather": (False if gather is None else "sync" if args.sync_gather else "overlapped (transport of step k on a side stream beside the next kernels, ring of %d slabs)" % args.ring),
                       "gather_bytes_per_rank": (None if slab is None else slab.nbytes),
                       "parallelism": "env-shard x%d" % world + (" (REHEARSAL: all ranks on one GPU, gloo)" if args.rehearse_one_gpu else ""),
                       "rccl_world_size": (dist.get_world_size() if dist is not None else None)},
            "timed_region": {"steps": args.steps, "whole_episodes": n_full, "spread_over_one_episode": n_spread,
                             "untimed_steps_between": untimed_advance, "clock": "HIP events per timed step" if (dist is None and not n_full) else "wall clock between barrier + synchronize" if n_spread == 0 or dist is not None else "wall clock (whole episodes) + HIP events (spread steps)"},
            "env_steps_per_s": (env_steps / elapsed if elapsed > 0 else None),
            "gpu_ms_per_step_rank0": gpu_ms / max(args.steps, 1),
            "shard_check": shard_check,
            "per_rank": (None if per_rank is None else {
                "wall_ms_per_step": [x[0] / max(args.steps, 1) * 1e3 for x in per_rank], "gpu_ms_per_step": [x[1] for x in per_rank],
                "slowest_over_fastest": max(x[0] for x in per_rank) / max(min(x[0] for x in per_rank), 1e-12)}),
            "sync_gather": sync_leg,
            "kernel_error_flags": err,
            "roofline": roofline,
            "full": args.full,
            "dumped_outputs": dumped,
        }
        if full is not None:  # the same kernel over one whole episode: the mean a training run sees
            out["ms_per_step_full_episode"] = full["ms_per_step"]  # (N > 1: rank 0's kernel alone, no transport)
            if "simd_isolation" in full:
                out["simd_isolation"] = full["simd_isolation"]
            out["value_full_episode"] = full["value"] if world == 1 else None
            if world == 1 and not robocup and not partial and not args.roofline_only:
                # the same episode on the plain grid: what SIMD isolation (3072 < E <= 4096 on a 256-CU device) is worth
                noiso = episode_leg(torch, device, args.workload, E, args.seed, n_players=n_players, no_isolation=True)
                out["value_no_isolation"], out["ms_per_step_no_isolation"] = noiso["value"], noiso["ms_per_step"]
        if args.full and world == 1 and not args.no_extra_legs and gather is None:
            env.close()
            out["other_configs"] = [episode_leg(torch, device, w, E, args.seed) for w in WORKLOADS if w != args.workload]
            if not args.no_cpu_baseline:   # the CPU port beside every MI355X figure, a bounded sample each
                for leg in out["other_configs"]:
                    wl = WORKLOADS[leg["workload"]]
                    leg["cpu_baseline"] = cpu_baseline(E, wl[2], 10, args.seed, wl[0], target_seconds=5.0, partial=wl[1])
            if args.workload == "driving":  # what the idle tail of a 4096-environment launch is worth (DESIGN.md "Batch size")
                out["throughput_vs_batch"] = [batch_leg(torch, device, e_, k_, args.seed)
                                              for e_, k_ in ((E, 2), (2 * E, 1), (4 * E, 1), (8 * E, 1))]
            out["plumbing_config0"] = plumbing_leg(torch, device, args.seed)
            if args.workload == "driving":
                out["arranger"] = arranger_leg(torch, device, E, args.seed)
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(E, n_players, A, args.seed, robocup, partial=partial)
            # BASELINE.md section 3 / SURVEY 8d name threads = os.cpu_count(): the same sample with one thread per logical CPU of the box
            # (on a GPU box whose cgroup grants 16 cores of an EPYC this OVERSUBSCRIBES the share; both figures are in the line)
            # (threads beyond the cgroup's core share are OVERSUBSCRIBED: with OMP_WAIT_POLICY=passive, set above, idle workers sleep, so
            #  the figure measures what the share delivers with that many threads - it cannot exceed the share's - and the note says so)
            allc = os.cpu_count() or 1
            try:
                allc = min(allc, len(os.sched_getaffinity(0)))
            except AttributeError:
                pass
            share = out["cpu_baseline"]["cores"]
            if allc == share:
                out["cpu_baseline_all_cores"] = dict(out["cpu_baseline"], note="threads = min(os.cpu_count(), affinity mask) = the cgroup's core share (%d): the same run" % share)
            else:
                over = cpu_baseline_oversubscribed(E, n_players, A, args.seed, robocup, partial, allc)
                out["cpu_baseline_all_cores"] = None if over is None else dict(
                    over, note="%d OpenMP threads (min of os.cpu_count() and the affinity mask) on a cgroup share of %d cores: OVERSUBSCRIBED %.0fx, run in a child "
                               "process with OMP_WAIT_POLICY=passive. Not a measurement of %d cores - read cpu_baseline (threads = the share) for the host's rate"
                               % (allc, share, allc / share, allc))
        elif args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = None
        sys.stdout.flush()
        os.dup2(real_stdout, 1)
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
