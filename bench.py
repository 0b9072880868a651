#!/usr/bin/env python
"""Benchmark of the NUTS hot path on MI355X (contract: see the round prompt, section 4).

Workload (BASELINE.json configs[1], SURVEY.md section 8d "C2-L hier-logit-10k"):
hierarchical logistic regression, n = 10 000 parameters (G=1248 groups x D=8),
N = 4 992 000 observation rows (X fp64 = 319.5 MB > 256 MiB LLC: HBM regime),
one NUTS chain per GPU, reference sampler defaults (target_accept 0.8,
max_treedepth 10 / 8 early, jitter+adapt_diag).  `--workload c3` runs BASELINE.json
configs[2] instead (MvNormal, full 2048 x 2048 covariance; cache-resident).

A "step" is one NUTS draw.  `--warmup W` tuning draws run untimed, then EXACTLY
`--steps K` post-warmup draws are timed between barrier + device synchronisation.

A plain run does only what the headline needs: set-up, the W warmup draws, the K
timed draws, and the one JSON line.  `--full` adds the legs that are not the
headline: the separate ESS run (`ess_run`) when K or W is too short for an ESS, the
CPU baseline, C3's chains on one GPU, and the oracle's own chains of this shape
(`oracle_convergence`).  `--dump-outputs DIR` writes what the last timed step
returned -- its draw and its sampler statistics -- as DIR/<name>.npy (float64); the
data and the seeds depend only on the arguments, so two builds can be compared
output for output.

value: BASELINE.json's metric names two numbers, effective samples/sec and leapfrog
steps/sec.  Effective samples/sec = sum over chains of the min-over-ALL-parameters
bulk-ESS of the K timed draws / max-over-ranks wall time -- it is only an estimate of
anything when the chain is tuned and K is a few hundred draws, so it is `value` when
K >= 200 and W >= 200; for shorter runs (e.g. a driver smoke run with K = 20) `value`
is the aggregate leapfrog steps/sec and the ESS fields are null (`value_is` says
which; `--full` fills them from `ess_run`).  `convergence` carries max R-hat, min /
median ESS and WHICH parameter has the minimum, so a small min-ESS can be traced to
the coordinate that does not mix.

roofline: dominant kernel = the hierarchical-logit row pass (csrc/rows_kernel.h /
rows_ga_kernel.h; with NUTS_GA_VARIANT=32 the persistent tree kernel of
rows_ga_tree.h, which runs a whole NUTS tree per launch); algorithmic bytes per pass
= 69 B/row x N (SURVEY.md 8d B_model: X row + y + int32 group id), divided by the
average duration of one pass measured with HIP events on the library stream during
the timed region (1 launch in 8 is bracketed by events; launches that drain after
the tree terminated are included, exactly as in the rocprofv3 summary under
profiles/; a tree launch is bracketed whole and its duration divided by the leaves
the tree ran).  4 of the 69 bytes
are bytes the kernel AVOIDS (group structure is read as G+1 row pointers), so
`frac_traffic` = PMC bytes / duration / peak is reported next to `frac`.
`traffic` = HBM bytes per launch from the rocprofv3 PMC passes of
tools/gpu_round.sh (2 x FETCH_SIZE + WRITE_SIZE, the gfx950 correction of
MI355X_MICROARCH.md), read from profiles/traffic.json together with the hash of the
kernel sources it was measured on (`traffic_build_matches`).

cpu_baseline (`--full`, rank 0, N=1 only): the oracle's reference-order leapfrog
(`oracle/ref_sampler.Leapfrog` = the restatement that reproduces the reference's
CpuLeapfrogIntegrator bitwise) over (i) the single-threaded gcc -O3 -march=native
restatement of logp+grad (stand-in for PyTensor's C linker, which cannot run here),
one chain on one core; (ii) the same, 8 chains concurrently on 8 pinned cores (the
reference's own configuration at 8 chains, mcmc.py:1203-1224); (iii) the NumPy
restatement, one core.  A bounded number of leapfrogs of the same workload each;
kind = "port".  Its ESS/s is DERIVED (CPU leapfrog/s x the GPU run's ESS per
leapfrog: the sampler is the same algorithm, so ESS per leapfrog is shared) -- the
measured quantity is leapfrog steps/s.
"""

from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ESS_MIN_DRAWS = 200


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=1000)
    ap.add_argument("--workload", default="c2", choices=["c2", "c3", "glm"],
                    help="c2 = hier-logit-10k (the headline), c3 = MvNormal 2048, glm = NUTS on configs[3]'s GLM (1 M rows x 512 covariates, the dense "
                         "linear-predictor node of csrc/glm_kernel.h) -- not the headline either")
    ap.add_argument("--glm-rows", type=int, default=1_000_000)
    ap.add_argument("--glm-cols", type=int, default=512)
    ap.add_argument("--glm-family", default="bernoulli", choices=["normal", "bernoulli", "poisson"])
    ap.add_argument("--rows-per-group", type=int, default=4000, help="4000 = C2-L (HBM regime), 80 = C2-S (cache resident)")
    ap.add_argument("--groups", type=int, default=1248)
    ap.add_argument("--variant", default=None, help="NOT the headline: the same rows under another model around them (pymc_amd.models.HIER_LOGIT_VARIANTS: "
                    "other hyper-priors, further variables) -- A/B of the generalised one-launch row pass against the benchmark's own model")
    ap.add_argument("--mvn-k", type=int, default=2048)
    ap.add_argument("--chains-per-gpu", type=int, default=4, help="--workload c3, one GPU: after the timed single-chain run, BASELINE configs[2]'s "
                    "4 chains on this GPU -- as independent engines and as a chain group (pymc_amd/chain_group.py) -- reported under "
                    "`chains_on_one_gpu` (0 or 1 disables; NOT part of `value`)")
    ap.add_argument("--seed", type=int, default=20160911)
    ap.add_argument("--cpu-leapfrogs", type=int, default=100, help="bounded CPU-baseline sample per leg (0 disables)")
    ap.add_argument("--draw-batch", type=int, default=int(os.environ.get("PYMC_AMD_DRAW_BATCH", "64")), help="post-tuning transitions per C call")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL; gloo only for tests)")
    ap.add_argument("--cpu-worker", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-worker-file", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--share-gpu", action="store_true", help="TEST ONLY: every rank uses GPU 0 (exercises the N > 1 logic on a 1-GPU box)")
    ap.add_argument("--stub-engine", action="store_true", help="TEST ONLY: no device work at all; drives launcher + gather + report on a CPU box")
    ap.add_argument("--launch-timeout", type=float, default=3600.0, help="self-launched ranks are stopped after this many seconds")
    ap.add_argument("--ess-tune", type=int, default=1000, help="warmup of the separate ESS chain run when --steps/--warmup are too short for an ESS (0 disables)")
    ap.add_argument("--ess-draws", type=int, default=1000)
    ap.add_argument("--ess-chains", type=int, default=8, help="chains of the ESS run on each GPU, one after the other (world == 1 only): min-ESS and "
                    "R-hat over several chains instead of a one-chain estimate (0 / 1: the single chain)")
    ap.add_argument("--full", action="store_true", help="also run what is not the headline: the separate ESS run (--ess-*), the CPU baseline "
                    "(--cpu-leapfrogs), C3's chains on one GPU (--chains-per-gpu), the oracle's own chains of this shape; a plain run times "
                    "the K steps and reports them")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write what the last timed step returned (its "
                    "draw and its sampler statistics) as DIR/<name>.npy, float64; ranks other than 0 add _rank<r> to the names")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


def kernel_source_hash():
    h = hashlib.sha1()
    d = os.path.join(ROOT, "pymc_amd", "csrc")
    for f in sorted(os.listdir(d)):
        with open(os.path.join(d, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:12]


# wall / CPU clocks of the draw and the warning object: not outputs of the computation
_DUMP_SKIP_STATS = ("perf_counter_diff", "perf_counter_start", "process_time_diff", "warning")
# NaN placeholders unless the potential estimates its mass matrix's eigenvalues (the diagonal one never does: quadpotential.py)
_DUMP_IF_ESTIMATED = ("largest_eigval", "smallest_eigval")


def dump_outputs(out_dir, rank, draw, stats):
    """`--dump-outputs DIR`: the last timed step's draw (one position, n float64) and its numeric sampler statistics, one .npy each."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {} if draw is None else {"draw": draw}
    for k, v in stats.items():
        if k in _DUMP_SKIP_STATS or not isinstance(v, (bool, int, float, np.bool_, np.number)):
            continue
        if k in _DUMP_IF_ESTIMATED and not np.isfinite(v):
            continue
        arrays[f"stat_{k}"] = v
    suffix = f"_rank{rank}" if rank else ""
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), np.asarray(a, dtype=np.float64))


# ---------------------------------------------------------------------------
# CPU baseline: reference-order leapfrogs on the host cores
# ---------------------------------------------------------------------------

def _cpu_leapfrogs(f, n, q, step_size, inv_mass, n_leap, core=None):
    from oracle import ref_sampler

    if core is not None:
        try:
            os.sched_setaffinity(0, {core})
        except Exception:
            pass
    pot = ref_sampler.DiagPotential(inv_mass)
    integ = ref_sampler.Leapfrog(pot, f)
    rng = np.random.default_rng(0 if core is None else core)
    s = integ.compute_state(np.array(q), rng.normal(size=n) / np.sqrt(inv_mass))
    t0 = time.perf_counter()
    for _ in range(n_leap):
        s = integ.step(step_size, s)
    return n_leap / (time.perf_counter() - t0)


def cpu_worker_main(args):
    """`bench.py --cpu-worker CORE --cpu-worker-file F`: one pinned process of the concurrent CPU leg (a fresh interpreter:
    nothing of the parent's HIP runtime is forked)."""
    from oracle import c_logit
    from pymc_amd import models

    try:
        import threadpoolctl

        threadpoolctl.threadpool_limits(1)
    except Exception:
        pass
    k = np.load(args.cpu_worker_file)
    spec = models.hier_logit(G=args.groups, D=8, rows_per_group=args.rows_per_group, seed=20160911)
    f = c_logit.CHierLogit(spec, so_path=str(k["so"]))
    lps = _cpu_leapfrogs(f, spec.n, k["q"], float(k["eps"]), k["inv_mass"], int(k["n_leap"]), args.cpu_worker)
    print(json.dumps({"core": args.cpu_worker, "leapfrog_steps_per_sec": lps}), flush=True)


def _measured_cpu_ess(args):
    """The oracle's own chains of this shape (committed fixture: four chains x (1000 + 1000), one per core, concurrently): min
    bulk-ESS of the pooled chains / their wall time -- measured where the fixture was made, stated with its host."""
    oc = oracle_convergence(args)
    if not oc or oc.get("oracle_ess_per_sec_measured") is None:
        return None
    return {"value": oc["oracle_ess_per_sec_measured"], "unit": "ESS/s (min bulk-ESS over all parameters, 4 chains on 4 cores concurrently, wall time incl. tuning)",
            "min_ess": oc["oracle_min_ess"], "wall_s": max(oc["oracle_wall_s_per_chain"]), "host": oc["oracle_wall_host"], "source": oc["source"]}


def cpu_baseline_c2(args, spec, q, step_size, inv_mass, n_leap, ess_per_leapfrog):
    import subprocess
    import tempfile

    from oracle import c_logit, ref_models

    try:
        import threadpoolctl

        threadpoolctl.threadpool_limits(1)
    except Exception:  # pragma: no cover
        pass
    so = c_logit.build_native()   # compiled for the box it is timed on
    t0 = time.perf_counter()
    lps_c1 = _cpu_leapfrogs(c_logit.CHierLogit(spec, so_path=so), spec.n, q, step_size, inv_mass, n_leap)
    # 8 chains concurrently, one process per chain pinned to one core (mcmc.py:1203-1224: blas_cores // cores = 1 thread each)
    ncore = min(8, os.cpu_count() or 1)
    n8 = max(10, n_leap // 3)
    per = []
    try:
        with tempfile.TemporaryDirectory() as td:
            wf = os.path.join(td, "w.npz")
            np.savez(wf, q=q, eps=step_size, inv_mass=inv_mass, n_leap=n8, so=so)
            procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-worker", str(c), "--cpu-worker-file", wf,
                                       "--groups", str(args.groups), "--rows-per-group", str(args.rows_per_group)],
                                      stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True) for c in range(ncore)]
            for p in procs:
                o, _ = p.communicate(timeout=600)
                per.append(json.loads(o.strip().splitlines()[-1])["leapfrog_steps_per_sec"])
    except Exception as e:  # pragma: no cover
        print(f"bench: concurrent CPU leg failed: {e}", file=sys.stderr)
    # NumPy restatement (what the graph would cost without a C linker), a shorter sample: it is several times slower
    n_np = max(4, n_leap // 12)
    lps_np = _cpu_leapfrogs(ref_models.SpecLogpGrad(spec), spec.n, q, step_size, inv_mass, n_np)
    dt = time.perf_counter() - t0
    ess_derived = None if ess_per_leapfrog is None else lps_c1 * ess_per_leapfrog
    return {
        "value": lps_c1 if ess_derived is None else ess_derived,
        "unit": "leapfrog steps/s" if ess_derived is None else "ESS/s (derived: measured leapfrog steps/s x the GPU run's ESS per leapfrog)",
        "leapfrog_steps_per_sec": lps_c1,
        "ess_per_sec_derived": ess_derived,
        "ess_per_sec_measured": _measured_cpu_ess(args),
        "cores": 1,
        "kind": "port",
        "host_cores_available": os.cpu_count(),
        "concurrent_8_chains": {
            "cores": len(per), "leapfrog_steps_per_sec_per_chain": [float(x) for x in per],
            "leapfrog_steps_per_sec_total": float(sum(per)), "leapfrogs_each": n8,
        },
        "numpy_variant": {"cores": 1, "leapfrog_steps_per_sec": lps_np, "leapfrogs": n_np},
        "sample": f"{n_leap} reference-order leapfrog steps of the same workload on one core (oracle integrator + single-threaded gcc -O3 "
        f"-march=native fused logp/grad, compiled on this box), then {n8} each in {len(per)} concurrent pinned processes, then {n_np} with the "
        f"NumPy logp/grad; {dt:.1f} s in all.  Restated reference CPU path (PyTensor unavailable)",
    }


def cpu_baseline_c3(spec, q, step_size, inv_mass, n_leap, what="SciPy Cholesky-solve logp/grad"):
    from oracle import ref_models

    try:
        import threadpoolctl

        threadpoolctl.threadpool_limits(1)
    except Exception:  # pragma: no cover
        pass
    t0 = time.perf_counter()
    lps = _cpu_leapfrogs(ref_models.SpecLogpGrad(spec), spec.n, q, step_size, inv_mass, n_leap)
    return {
        "value": lps, "unit": "leapfrog steps/s (one chain on one host core)", "leapfrog_steps_per_sec": lps, "cores": 1, "kind": "port",
        "host_cores_available": os.cpu_count(),
        "sample": f"{n_leap} reference-order leapfrog steps (oracle integrator + {what}, BLAS threads = 1) in {time.perf_counter() - t0:.1f} s",
    }


# ---------------------------------------------------------------------------
# `python bench.py --gpus N` without a launcher: one process per chain / GPU, the parent collects
# (the reference's layout for cores > 1: pymc/sampling/parallel.py:477-589, mcmc.py:1203-1224)
# ---------------------------------------------------------------------------

def visible_gpus():
    """Devices this process could hand to ranks (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES respected by the runtime)."""
    try:
        import torch

        return int(torch.cuda.device_count()) if torch.cuda.is_available() else 0
    except Exception:
        return 0


def _free_port():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args, argv):
    """No WORLD_SIZE in the environment and --gpus N > 1: start N copies of this script as ranks 0..N-1 (RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_* exactly as `torch.distributed.run` would set them), rank r on GPU r, RCCL group over the N devices;
    rank 0 prints the one JSON line.  Refuses (exit code 2) when fewer than N devices are visible -- a silent 1-GPU run under
    `--gpus 8` would be a wrong scaling point.  Returns the exit code."""
    import subprocess

    n = args.gpus
    if not (args.stub_engine or args.share_gpu):
        have = visible_gpus()
        if have < n:
            print(f"bench: --gpus {n} requested but {have} GPU(s) visible; refusing to run fewer ranks than asked "
                  "(--share-gpu puts every rank on GPU 0 for TESTING the launch path)", file=sys.stderr)
            return 2
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   LOCAL_WORLD_SIZE=str(n), PYMC_AMD_BENCH_SELF_LAUNCHED="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    deadline = time.time() + args.launch_timeout
    alive = list(procs)
    while alive:
        for p in list(alive):
            code = p.poll()
            if code is None:
                continue
            alive.remove(p)
            if code != 0:
                rc = rc or code
        if (rc != 0 or time.time() > deadline) and alive:
            # one rank died (or the run overran): the others would wait in a collective for ever -- stop exactly the processes
            # started here
            for p in alive:
                p.kill()
            for p in alive:
                p.wait()
            rc = rc or 124
            break
        time.sleep(0.05)
    return rc


class _StubChain:
    """TEST ONLY (`--stub-engine`): stands where one rank's device chain stands so that the launcher, the process group, the
    gather and the report can be driven on a box without a GPU (tests/test_bench_launch.py).  Fabricates tree sizes; measures
    nothing."""

    def __init__(self, rank):
        self.rank = rank

    def run(self, K):
        if os.environ.get("PYMC_AMD_BENCH_STUB_FAIL_RANK") == str(self.rank):
            sys.exit(3)          # (a rank that dies: the launcher must stop the others, which wait in a collective)
        rng = np.random.default_rng(1000 + self.rank)
        tree = rng.choice([15, 31, 63], size=K).astype(float)
        time.sleep(0.002 * K)
        return tree


def run_rank(args):
    """One rank = one chain on one GPU: W untimed tuning draws, K timed draws between barriers; returns what rank 0 needs."""
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    stub = args.stub_engine
    import torch

    dist = None
    rccl = {"group": None, "ranks": 0, "why_not": None}
    if args.share_gpu or stub:
        local = 0
        if os.environ.get("PYMC_AMD_BENCH_STUB_TRY_RCCL") != "1":   # (the test of the fall-back below leaves RCCL requested on a box without a GPU)
            args.backend = "gloo"   # RCCL refuses two ranks on one device ("Duplicate GPU detected")
    if world > 1:
        import torch.distributed as dist

        # The control plane -- barriers around the timed region, the gather of the ranks' small result records -- is a gloo group
        # on the host: it cannot fail for a reason that has to do with the GPU runtimes, and chains exchange
        # nothing on the data path.  RCCL is brought up NEXT TO it, as a second group, for what the north star gives it (the final
        # gather of device-resident results, the opt-in pooled adaptation); it is probed with one all-reduce whose answer every
        # rank checks, and the ranks agree through the gloo group whether it is usable.  If it is not, the run goes on over gloo
        # and says so in `collective_backend` instead of dying in the launcher.
        from pymc_amd.parallel import init_process_groups, rccl_group

        if not stub:
            torch.cuda.set_device(local)
        status = init_process_groups(args.backend, local_device=local)    # (pymc_amd/parallel.py: the same bring-up `sample()` launches use)
        rccl.update(group=rccl_group(), ranks=status["ranks"], why_not=status["why_not"])
        if args.backend == "nccl" and not rccl["ranks"]:
            args.backend = "gloo"
    elif not stub:
        torch.cuda.set_device(0)

    def barrier():
        if not stub:
            torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        if not stub:
            torch.cuda.synchronize()

    W, K = args.warmup, args.steps
    c3 = args.workload == "c3"
    glm = args.workload == "glm"
    meta = {}
    if stub:
        chain = _StubChain(rank)
        barrier()
        t0 = time.perf_counter()
        tree = chain.run(K)
        barrier()
        dt = time.perf_counter() - t0
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, rank, None, {"tree_size": tree[-1]})
        leap = float(tree.sum())
        vec = [dt, 0.0, leap, 0.0, 0.0, 0.0, 0.0]        # (no kernel: the roofline block of a stub line reads 0)
        conv, ess_run = None, None
        meta = dict(alg_bytes=344448000, n=10000, N=4992000, workload="STUB ENGINE (test of the launch path; nothing measured)", kernel="stub",
                    schedule="stub", traffic_ok=False)
        ess_ok = False
        draws = step = spec = None
    else:
        from pymc_amd import models
        from pymc_amd.sampling import init_nuts, sample_draws
        from pymc_amd.step import get_random_generator
        from pymc_amd.stats import ess_bulk_many, rhat_many

        t_setup0 = time.perf_counter()
        if c3:
            spec = models.mvnormal(n=args.mvn_k)
            N = 0
        elif glm:
            spec = models.glm_nuts(N=args.glm_rows, P=args.glm_cols, family=args.glm_family)
            N = args.glm_rows
        else:
            if args.variant:
                spec = models.hier_logit_variant(args.variant, G=args.groups, D=8, rows_per_group=args.rows_per_group, seed=20160911)
            else:
                spec = models.hier_logit(G=args.groups, D=8, rows_per_group=args.rows_per_group, seed=20160911)
            N = spec.logit_rows.X.shape[0]
        t_data = time.perf_counter() - t_setup0          # this rank's synthetic data (every rank generates its own replica)
        chains = world
        rngs = get_random_generator(args.seed).spawn(chains)  # mcmc.py:907-908
        seed_list = [int(r.integers(2**30)) for r in rngs]
        t_setup1 = time.perf_counter()
        points, step = init_nuts(spec, init="jitter+adapt_diag", chains=chains, random_seed_list=seed_list, device=local)
        t_init = time.perf_counter() - t_setup1          # layout of X, upload, engine handles, the jittered start points
        alg_bytes = step._logp_dlogp_func.algorithmic_bytes
        os.environ["PYMC_AMD_DRAW_BATCH"] = str(args.draw_batch)
        initial_state = step.sampling_state
        # the per-chain loop of `_iter_sample` (mcmc.py:1503-1583), split at the end of tuning so that exactly the K
        # post-warmup transitions sit between the two barriers
        step.setup_chain(rngs[rank], W, K)
        step.tune = bool(W)
        step.reset_tuning()
        point = points[rank]
        step.iter_count = 0
        _, _, point = sample_draws(step, point, W)
        step.stop_tuning()

        step.profile(True)
        barrier()
        t0 = time.perf_counter()
        draws, stats_list, point = sample_draws(step, point, K)
        barrier()
        dt = time.perf_counter() - t0
        dom_ms, dom_n, _ = step.profile_read()
        step.profile(False)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, rank, draws[-1], stats_list[-1])
        tree = np.array([s["tree_size"] for s in stats_list])
        n_div = int(sum(bool(s["diverging"]) for s in stats_list))
        leap = float(tree.sum())

        names = []
        for v in spec.vars:
            names += [f"{v.value_name}[{k}]" for k in range(v.size)]

        def convergence(d, n_div_):
            ess = ess_bulk_many(d[None])
            rh = rhat_many(d[None])          # split R-hat of the one chain this rank ran
            j = int(np.nanargmin(ess))
            cv = {"min_ess": float(ess[j]), "min_ess_param_index": j, "min_ess_param": names[j], "median_ess": float(np.median(ess)),
                  "ess_5pct": float(np.percentile(ess, 5)), "rhat_max": float(np.nanmax(rh)), "rhat_max_param": names[int(np.nanargmax(rh))],
                  "rhat_of_min_ess_param": float(rh[j]), "n_params": int(spec.n), "divergences": n_div_}
            if not c3 and not glm:
                # The non-centred parametrisation SURVEY 8 prescribes leaves (mu_d, mean_g z_{g,d}) on a ridge when every group has
                # thousands of rows: the combination the likelihood identifies, beta_bar_d = mu_d + sigma_d
                # mean_g z_{g,d}, is reported next to the per-coordinate minimum so that the two can be told apart.
                v = {x.name: x for x in spec.vars}
                D_ = v["mu"].size
                mu_ = d[:, v["mu"].offset : v["mu"].offset + D_]
                sg_ = np.exp(d[:, v["sigma"].offset : v["sigma"].offset + D_])
                zbar = d[:, v["z"].offset : v["z"].offset + v["z"].size].reshape(len(d), -1, D_).mean(axis=1)
                eb = ess_bulk_many((mu_ + sg_ * zbar)[None])
                cv["identified_combination"] = {"what": "beta_bar_d = mu_d + sigma_d * mean_g z[g, d]", "min_ess": float(eb.min()),
                                                "median_ess": float(np.median(eb)), "corr_mu_zbar_d0": float(np.corrcoef(mu_[:, 0], zbar[:, 0])[0, 1])}
            return cv

        ess_ok = K >= ESS_MIN_DRAWS and W >= ESS_MIN_DRAWS
        conv = convergence(draws, n_div) if ess_ok else None
        min_ess = conv["min_ess"] if ess_ok else 0.0
        vec = [dt, min_ess, leap, dom_ms, float(dom_n), t_data, t_init]

        # The metric's other half when the timed region is too short to carry it (a driver run with K = 20): a SEPARATE whole chain
        # of ess_tune + ess_draws transitions from a fresh sampling state, timed INCLUDING its warmup as the reference's benchmark
        # does (benchmarks/benchmarks/benchmarks.py:180-198: min ESS / total sampling time).  Reported under "ess_run"; it
        # never enters `value`, `ms_per_step` or the roofline block, which describe exactly the K timed steps above.
        ess_run = None
        if args.full and not ess_ok and args.ess_draws >= ESS_MIN_DRAWS and args.ess_tune >= ESS_MIN_DRAWS:
            from pymc_amd.sampling import sample_chain

            step.sampling_state = initial_state
            barrier()
            t1 = time.perf_counter()
            d_all, st_all = sample_chain(step, points[rank], get_random_generator(args.seed).spawn(chains)[rank], args.ess_tune, args.ess_draws)
            barrier()
            wall = time.perf_counter() - t1
            st_post = st_all[args.ess_tune:]
            cv = convergence(d_all[args.ess_tune:], int(sum(bool(s_["diverging"]) for s_ in st_post)))
            ess_run = {"wall_s": wall, "min_ess": cv["min_ess"], "leapfrogs_post_warmup": float(sum(s_["tree_size"] for s_ in st_post)),
                       "leapfrogs_total": float(sum(s_["tree_size"] for s_ in st_all)),
                       "sampling_s_post_warmup": float(sum(s_["perf_counter_diff"] for s_ in st_post)),
                       "step_size_bar": float(st_all[-1]["step_size_bar"]), "convergence": cv}
            if world == 1 and args.ess_chains > 1:
                # The same run with several chains on this GPU (the reference's `pm.sample(chains=4)`, mcmc.py:1385-1430), so that
                # min-ESS and R-hat are multi-chain estimates -- the reference's benchmark divides the ESS of ALL chains by the total
                # sampling time (benchmarks.py:180-198).  Round 5: the chains run CONCURRENTLY as a chain group where the engine can
                # merge their leapfrog launches (the group-aligned row pass streams X once for up to EIGHT chains standing at a leaf -- BASELINE
                # configs[1]'s eight --, csrc/rows_gal_kernel.h; draws bitwise those of the chains alone), one after the other otherwise.
                from pymc_amd.sampling import sample

                t2 = time.perf_counter()
                res_mc = sample(draws=args.ess_draws, tune=args.ess_tune, chains=args.ess_chains, model=spec, init="jitter+adapt_diag",
                                random_seed=args.seed + 1, device=local)
                wall_mc = time.perf_counter() - t2
                res_mc["step"].close()
                stack = res_mc["draws"]
                ess_c, rh_c = ess_bulk_many(stack), rhat_many(stack)
                ident = None
                if not c3 and not glm:
                    # the combination the likelihood identifies (see `convergence`): THIS is what has converged in such a run -- its
                    # multi-chain ESS over the same wall time next to the minimum over the 10 000 raw coordinates, which has not
                    v_ = {x.name: x for x in spec.vars}
                    D_ = v_["mu"].size
                    mu_ = stack[:, :, v_["mu"].offset : v_["mu"].offset + D_]
                    sg_ = np.exp(stack[:, :, v_["sigma"].offset : v_["sigma"].offset + D_])
                    zb_ = stack[:, :, v_["z"].offset : v_["z"].offset + v_["z"].size].reshape(stack.shape[0], stack.shape[1], -1, D_).mean(axis=2)
                    bb_ = mu_ + sg_ * zb_
                    eb_, rb_ = ess_bulk_many(bb_), rhat_many(bb_)
                    ident = {"what": "beta_bar_d = mu_d + sigma_d * mean_g z[g, d], d = 0..7 (what the likelihood identifies)", "min_ess": float(eb_.min()),
                             "rhat_max": float(np.nanmax(rb_)), "ess_per_sec": float(eb_.min() / res_mc["wall_time"])}
                n_l = res_mc["lockstep_launches"]
                lf_post = float(sum(s_["tree_size"] for c_ in range(args.ess_chains) for s_ in res_mc["stats"][c_]))
                ess_run["multi_chain"] = {
                    "chains": args.ess_chains,
                    "how": ("concurrently as a chain group: one launch per leapfrog streams the data once for the chains standing at a leaf"
                            if n_l else "one after the other on this GPU") + ", each tuned on its own from a jittered start",
                    "wall_s_total": float(wall_mc), "sampling_s": float(res_mc["wall_time"]), "sampling_s_post_warmup": float(res_mc["sampling_time"]),
                    "min_ess": float(ess_c.min()), "median_ess": float(np.median(ess_c)), "rhat_max": float(np.nanmax(rh_c)),
                    "n_rhat_gt_1.01": int((rh_c > 1.01).sum()), "ess_per_sec": float(ess_c.min() / res_mc["wall_time"]),
                    "aggregate_leapfrog_steps_per_sec_post_warmup": lf_post / float(res_mc["sampling_time"]),
                    "launches_by_chains_carried": n_l[1:] if n_l else None,
                    "mean_chains_per_launch": (sum(c_ * n_l[c_] for c_ in range(1, len(n_l))) / max(1, sum(n_l[1:]))) if n_l else None,
                    # a converged quantity of the same run
                    "identified_combination": ident,
                }
        if c3:
            workload = f"C3 mvn-{args.mvn_k}: MvNormal, full {args.mvn_k}x{args.mvn_k} covariance, n={spec.n}"
            aligned = int(step._logp_dlogp_func.model_scalar("mvn_row_aligned"))
            kernel = (f"k_mvn_aligned<{aligned}> (precision mat-vec whose workgroups also finish the leapfrog: one launch per leapfrog"
                      if aligned else "k_mvn_matvec (precision mat-vec") + \
                "; cache-resident: 33.5 MB < 256 MiB Infinity Cache -- the HBM line does not bound it)"
        elif glm:
            workload = (f"GLM NUTS (configs[3]'s model under NUTS): N={args.glm_rows} observations x P={args.glm_cols} covariates, {args.glm_family} family, "
                        f"alpha + X beta, n={spec.n}")
            kernel = (f"k_glm_rows (one fused forward + backward read of X per leapfrog, row stride {int(step._logp_dlogp_func.model_scalar('glm_row_stride'))} doubles, "
                      f"{int(step._logp_dlogp_func.model_scalar('glm_workgroups'))} workgroups; csrc/glm_kernel.h)")
        else:
            workload = f"C2-{'L' if args.rows_per_group >= 1000 else 'S'} hier-logit-10k: G={args.groups} D=8 rows={N} n={spec.n}"
            if args.variant:
                workload += (f" [VARIANT {args.variant}: not the headline model; {int(step._logp_dlogp_func.model_scalar('rows_aux_workgroups'))} "
                             "auxiliary workgroup(s) per launch, csrc/rows_aux.h]")
            kernel = "hierarchical-logit row pass (k_rows_ga / k_rows_gb / k_rows)"
        schedule = ("persistent tree kernel: one launch per NUTS tree (csrc/rows_ga_tree.h)" if step._scalar("tree_kernel") else
                    f"group-block row pass: one launch per leapfrog, {int(step._logp_dlogp_func.model_scalar('rows_group_block'))} groups per workgroup, block "
                    "partials cross the kernel boundary, control work folded into the next row pass, also across doublings (csrc/rows_gb_kernel.h)"
                    if (not c3 and step._logp_dlogp_func.model_scalar("rows_group_block")) else
                    "group-aligned row pass: one launch per leapfrog, control work folded into the next row pass, also across doublings "
                    "(csrc/rows_ga_kernel.h)" if (not c3 and step._logp_dlogp_func.model_scalar("rows_group_aligned")) else
                    "row-aligned MvNormal pass: one launch per leapfrog, control work folded into the next launch, also across doublings "
                    "(csrc/kernels.h, k_mvn_aligned)" if (c3 and step._logp_dlogp_func.model_scalar("mvn_row_aligned")) else
                    "four launches per leapfrog: the fused pass over X, the totals of its records, the O(n) kernel, the control kernel (csrc/glm_kernel.h)" if glm else
                    "two launches per leapfrog (data pass + O(n) kernel), control work folded into the next data pass (csrc/kernels.h)")
        meta = dict(alg_bytes=alg_bytes, n=int(spec.n), N=N, workload=workload, kernel=kernel, schedule=schedule, traffic_ok=True)

    if dist is not None:
        # the final gather: over RCCL from device memory when it is up (one 40-byte record per rank here; `sample(...)` gathers
        # the draws the same way, pymc_amd/sampling.py), over the host group otherwise
        if rccl["group"] is not None:
            t = torch.tensor(vec, dtype=torch.float64, device=torch.device("cuda", local))
            allt = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(allt, t, group=rccl["group"])
            torch.cuda.synchronize()
        else:
            t = torch.tensor(vec, dtype=torch.float64)
            allt = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(allt, t)
        allv = torch.stack(allt).cpu().numpy()
        convs = [None] * world
        dist.all_gather_object(convs, conv)
        ess_runs = [None] * world
        dist.all_gather_object(ess_runs, ess_run)
    else:
        allv = np.array([vec])
        convs = [conv]
        ess_runs = [ess_run]
    if rank == 0:
        out = report(args, world, allv, convs, ess_runs, meta, ess_ok, rccl)
        if args.full and world == 1 and args.cpu_leapfrogs > 0 and not stub:
            inv_mass = step._vector("var")
            eps = float(step._scalar("step_size"))
            if c3 or glm:
                # (a GLM leapfrog on one core is two passes over 4 GB of X: a bounded sample of 20)
                out["cpu_baseline"] = (cpu_baseline_c3(spec, draws[-1], eps, inv_mass, min(args.cpu_leapfrogs, 20), "NumPy X @ beta / X^T r logp/grad") if glm else
                                       cpu_baseline_c3(spec, draws[-1], eps, inv_mass, args.cpu_leapfrogs))
            else:
                out["cpu_baseline"] = cpu_baseline_c2(args, spec, draws[-1], eps, inv_mass, args.cpu_leapfrogs,
                                                      (vec[1] / max(leap, 1.0)) if ess_ok else
                                                      (ess_run["min_ess"] / max(ess_run["leapfrogs_total"], 1.0)) if ess_run else None)
        if args.full and c3 and world == 1 and not stub and 2 <= args.chains_per_gpu <= 4:
            try:
                out["chains_on_one_gpu"] = chains_on_one_gpu(args, spec, local)
            except Exception as e:     # (an extra leg: the line of the timed region is printed whatever happens here)
                out["chains_on_one_gpu"] = {"error": f"{type(e).__name__}: {e}"}
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def chains_on_one_gpu(args, spec, device, tune=500, draws=1000):
    """BASELINE configs[2] says `"chains": 4`: the same model's four chains on ONE GPU, from host threads -- each with an engine and
    a stream of its own, and as a chain group whose members share one launch per leapfrog (csrc/mvn_multi_kernel.h; the draws are
    bitwise the independent chains').  Aggregate leapfrog steps/s over the post-tuning draws = all chains' leapfrogs / the slowest
    worker's sampling time; `ess_per_sec` = the pooled four-chain bulk-ESS of the worst parameter over the same time (BASELINE's
    metric for this config).  A separate, bounded run: not part of `value`."""
    from pymc_amd.sampling import sample
    from pymc_amd.stats import ess_bulk_many, rhat_many

    out, ref = {"chains": args.chains_per_gpu, "tune": tune, "draws": draws}, None
    for mode, lockstep in (("independent_engines", False), ("chain_group", True)):
        res = sample(draws=draws, tune=tune, chains=args.chains_per_gpu, model=spec, init="jitter+adapt_diag", random_seed=args.seed, device=device,
                     cores=args.chains_per_gpu, lockstep=lockstep)
        res["step"].close()
        lf = sum(int(s_["tree_size"]) for c in range(args.chains_per_gpu) for s_ in res["stats"][c])
        n = res["lockstep_launches"]
        ess = ess_bulk_many(res["draws"])
        out[mode] = {"leapfrog_steps_per_sec": lf / res["sampling_time"], "sampling_time_s": res["sampling_time"],
                     "min_ess": float(ess.min()), "ess_per_sec": float(ess.min()) / res["sampling_time"], "rhat_max": float(rhat_many(res["draws"]).max()),
                     "launches_by_chains_carried": n[1:] if n else None,
                     "mean_chains_per_launch": (sum(c * n[c] for c in range(1, 5)) / max(1, sum(n[1:]))) if n else None}
        if ref is None:
            ref = res["draws"]
        else:
            out["draws_bitwise_equal"] = bool(np.array_equal(ref, res["draws"]))
    # sixteen chains as a WIDE group: every merged launch through the matrix cores (csrc/mvn_mfma_kernel.h, v_mfma_f64_16x16x4_f64)
    wide = 16
    res = sample(draws=draws, tune=tune, chains=wide, model=spec, init="jitter+adapt_diag", random_seed=args.seed, device=device, cores=wide, lockstep=True)
    res["step"].close()
    lf = sum(int(s_["tree_size"]) for c in range(wide) for s_ in res["stats"][c])
    n = res["lockstep_launches"]
    ess = ess_bulk_many(res["draws"])
    out["wide_chain_group_mfma"] = {"chains": wide, "leapfrog_steps_per_sec": lf / res["sampling_time"], "sampling_time_s": res["sampling_time"],
                                    "min_ess": float(ess.min()), "ess_per_sec": float(ess.min()) / res["sampling_time"],
                                    "rhat_max": float(rhat_many(res["draws"]).max()), "launches_by_chains_carried": n[1:] if n else None,
                                    "mean_chains_per_launch": (sum(c * n[c] for c in range(1, len(n))) / max(1, sum(n[1:]))) if n else None}
    return out


def oracle_convergence(args):
    """What the CPU ORACLE's own four chains of the benchmarked shape look like (tests/golden/c2l_chains.npz, written by
    tests/golden/make_c2_fixtures.py from oracle/ref_sampler.py: a committed fixture, read as data -- nothing of oracle/ is
    imported): if the reference sampler shows the same R-hat on this model, a large R-hat of the device chain is the model."""
    if args.workload != "c2" or args.groups != 1248 or args.variant:
        return None
    f = os.path.join(ROOT, "tests", "golden", "c2l_chains.npz" if args.rows_per_group == 4000 else "c2s_chains.npz" if args.rows_per_group == 80 else "-")
    if not os.path.exists(f):
        return None
    k = np.load(f)
    tune = int(k["config"][3])
    return {"source": os.path.relpath(f, ROOT), "chains": int(k["config"][5]), "tune": tune, "draws": int(k["config"][4]),
            "oracle_rhat_max": float(k["rhat"].max()), "oracle_n_rhat_gt_1.01": int((k["rhat"] > 1.01).sum()),
            "oracle_min_ess": float(k["ess_bulk"].min()), "oracle_median_ess": float(np.median(k["ess_bulk"])),
            "oracle_mean_tree_size": float(k["stat_tree_size"][:, tune:].mean()),
            "oracle_step_size_bar": [float(x) for x in k["stat_step_size_bar"][:, -1]],
            # MEASURED CPU ESS/s of the restated reference sampler: the chains' own wall time, tuning included,
            # on the host that generated the fixture (not this box: a 2.7-hour chain is not a bench leg) -- min bulk-ESS over
            # all parameters of the pooled chains / the time the concurrently running chains took
            "oracle_wall_s_per_chain": [float(x) for x in k["wall_s"]] if "wall_s" in k.files else None,
            "oracle_wall_host": str(k["wall_host"]) if "wall_host" in k.files else None,
            "oracle_ess_per_sec_measured": float(k["ess_bulk"].min() / k["wall_s"].max()) if "wall_s" in k.files else None}


def report(args, world, allv, convs, ess_runs, meta, ess_ok, rccl=None):
    """The one JSON line (rank 0)."""
    K, W = args.steps, args.warmup
    c3 = args.workload == "c3"
    glm = args.workload == "glm"
    alg_bytes, n = meta["alg_bytes"], meta["n"]
    T = float(allv[:, 0].max())
    leap_total = float(allv[:, 2].sum())
    lps_total = leap_total / T
    lps_chain = allv[:, 2] / allv[:, 0]
    dom_avg_ms = float(allv[:, 3].sum() / max(allv[:, 4].sum(), 1))
    ess_total = float(allv[:, 1].sum()) if ess_ok else None
    achieved = alg_bytes / (dom_avg_ms * 1e-3) / 1e9 if dom_avg_ms > 0 else 0.0
    traffic, traffic_src, traffic_match = None, None, None
    tj = os.path.join(ROOT, "profiles", "traffic.json")
    if meta["traffic_ok"] and not c3 and not glm and not args.variant and os.path.exists(tj) and args.rows_per_group == 4000 and args.groups == 1248:
        tr = json.load(open(tj))
        traffic, traffic_src = tr["k_rows_bytes_per_launch"], tr["source"]
        traffic_match = tr.get("kernel_source_hash") == kernel_source_hash()
    tjg = os.path.join(ROOT, "profiles", "traffic_glm.json")
    if meta["traffic_ok"] and glm and os.path.exists(tjg) and args.glm_rows == 1_000_000 and args.glm_cols == 512:
        tr = json.load(open(tjg))
        traffic, traffic_src = tr["k_glm_rows_bytes_per_launch"], tr["source"]
        traffic_match = tr.get("kernel_source_hash") == kernel_source_hash()
    tj3 = os.path.join(ROOT, "profiles", "traffic_c3.json")
    if meta["traffic_ok"] and c3 and os.path.exists(tj3) and args.mvn_k == 2048:
        tr = json.load(open(tj3))
        traffic, traffic_src = tr["k_mvn_aligned_bytes_per_launch"], tr["source"]
        traffic_match = tr.get("kernel_source_hash") == kernel_source_hash()
    # the same launch timed by rocprofv3's kernel trace (no marker packets around it: the HIP events that bracket a launch here put
    # two of them on the stream, which stretches the bracketed launch by ~2 us -- VERDICT r04 weak 4), for the committed kernel
    # sources: `profiles/launch_time.json`, written by tools/rocpd_summary.py --launch-time from the round's profile run
    lt, lt_match = None, None
    ltj = os.path.join(ROOT, "profiles", "launch_time_c3.json" if c3 else "launch_time_glm.json" if glm else "launch_time.json")
    shape_ok = (args.mvn_k == 2048) if c3 else (args.glm_rows == 1_000_000 and args.glm_cols == 512) if glm else \
        (not args.variant and args.rows_per_group == 4000 and args.groups == 1248)
    if meta["traffic_ok"] and shape_ok and os.path.exists(ltj):
        lt = json.load(open(ltj))
        lt_match = lt.get("kernel_source_hash") == kernel_source_hash()
    leap_bytes = alg_bytes + 144 * n
    setup = {"what": "seconds before the first draw, per rank: this rank's synthetic data; layout + upload + engine handles + jittered starts",
             "data_s_per_rank": [float(x) for x in allv[:, 5]], "engine_s_per_rank": [float(x) for x in allv[:, 6]]} if allv.shape[1] >= 7 else None
    er = [e for e in ess_runs if e]
    ess_run = None
    if er and len(er) == world:
        wall = max(e["wall_s"] for e in er)
        ess_run = {
            "what": f"a separate whole chain per GPU, {args.ess_tune} tune + {args.ess_draws} draws from a fresh sampling state, timed INCLUDING warmup "
                    "(benchmarks/benchmarks/benchmarks.py:180-198); not part of the K timed steps `value` describes",
            "ess_per_sec": sum(e["min_ess"] for e in er) / wall, "wall_s": wall, "min_ess_per_chain": [e["min_ess"] for e in er],
            "leapfrog_steps_per_sec_post_warmup_per_chain": [e["leapfrogs_post_warmup"] / max(e["sampling_s_post_warmup"], 1e-9) for e in er],
            "mean_tree_size_post_warmup": sum(e["leapfrogs_post_warmup"] for e in er) / (args.ess_draws * world),
            "step_size_bar": [e["step_size_bar"] for e in er], "convergence": [e["convergence"] for e in er],
            "multi_chain": er[0].get("multi_chain") if world == 1 else None,
            "oracle": oracle_convergence(args),
        }
    return {
        "metric": "effective samples/sec (and leapfrog steps/sec), 10k-param hierarchical logistic regression, one NUTS chain per GPU"
        if not (c3 or glm) else "leapfrog steps/sec (and effective samples/sec), MvNormal 2048, one NUTS chain per GPU" if c3 else
        "leapfrog steps/sec (and effective samples/sec), GLM with 1M observations x 512 covariates under NUTS, one chain per GPU",
        "value": (ess_total / T) if ess_ok else lps_total,
        "unit": "ESS/s (aggregate over chains; min-over-all-parameters bulk-ESS)" if ess_ok else "leapfrog steps/s (aggregate over chains)",
        "value_is": "ess_per_sec" if ess_ok else f"leapfrog_steps_per_sec (ESS needs steps >= {ESS_MIN_DRAWS} and warmup >= {ESS_MIN_DRAWS}; see ess_run)",
        "n_gpus": world,
        "steps": K,
        "warmup": W,
        "ms_per_step": 1e3 * T / K,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {
            "workload": meta["workload"],
            "chains": world,
            "parallelism": f"{world} independent chain(s), one per GPU, no data-path collective",
            "sampler": "NUTS target_accept=0.8 max_treedepth=10 init=jitter+adapt_diag",
        },
        "launch": ("self-launched: bench.py started one process per GPU" if os.environ.get("PYMC_AMD_BENCH_SELF_LAUNCHED") else
                   "launched by torch.distributed.run" if world > 1 else "single process"),
        "collective_backend": None if world == 1 else ("rccl (final gather; barriers and result records over a gloo host group)" if (rccl and rccl["ranks"]) else
                                                       "gloo" + (f" (RCCL could not be brought up: {rccl['why_not']})" if (rccl and rccl["why_not"]) else "")),
        # ranks that answered the RCCL probe (an all-reduce of ones that must sum to the world size on every rank)
        "rccl_ranks": int(rccl["ranks"]) if (rccl and world > 1) else 0,
        "schedule": meta["schedule"],
        "leapfrog_steps_per_sec": lps_total,
        "leapfrog_steps_per_sec_per_chain": [float(x) for x in lps_chain],
        "leapfrog_frac_per_chain": [float(leap_bytes * x / 8.0e12) for x in lps_chain],
        "ess_per_sec": (ess_total / T) if ess_ok else (ess_run["ess_per_sec"] if ess_run else None),
        "ess_per_sec_is": "the K timed steps" if ess_ok else ("ess_run (separate chain, wall time incl. warmup)" if ess_run else None),
        "ess_per_chain": [float(x) for x in allv[:, 1]] if ess_ok else None,
        "convergence": convs if ess_ok else None,
        "oracle_convergence": oracle_convergence(args) if (ess_ok and args.full) else None,
        "ess_run": ess_run,
        "setup": setup,
        "mean_tree_size": leap_total / (K * world),
        "roofline": {
            "bound": "hbm",
            "kernel": meta["kernel"],
            "achieved": achieved,
            "peak": 8000.0,
            "unit": "GB/s",
            "frac": achieved / 8000.0,
            "frac_of_achievable_6.3TBps": achieved / 6300.0,
            "algorithmic_bytes_per_launch": alg_bytes,
            "algorithmic_bytes_note": None if c3 else "8 N P: one read of the fp64 design matrix per logp + gradient (y: 8 N more, not counted)" if glm else "69 B/row = 64 (X) + 1 (y) + 4 (int32 group id); the kernel reads G+1 row pointers instead of the "
            "group ids, so 4 of the 69 are bytes it avoids -- frac_traffic prices the bytes actually moved",
            "avg_launch_ms": dom_avg_ms,
            "avg_launch_ms_is": ("HIP events on the kernel's own stream inside the timed region.  Inside a tree, doublings of 16 leaves or more -- back-to-back "
                                 "launches of this kernel -- are bracketed WHOLE (two marker packets per run, not per launch) and the time divided by the "
                                 "launches covered; runs that contain launches drained behind a finished tree are dropped; shallower trees: single launches"),
            "launches_timed": int(allv[:, 4].sum()),   # (passes over the data covered by the bracketed launches)
            # the figure must be consistent with the step time it is part of: (launches per step) x (average launch) <= ms_per_step
            "launches_per_step_x_avg_launch_ms": (leap_total / (K * world)) * dom_avg_ms,
            "consistent_with_ms_per_step": bool((leap_total / (K * world)) * dom_avg_ms <= 1e3 * T / K * 1.001),
            # the kernel trace's figure for the same launch, and the fraction it gives (consistent with ms_per_step: launches x median <= step)
            "rocprof_launch_us_median": lt["median_us"] if lt else None,
            "rocprof_launch_us_mean": lt["mean_us"] if lt else None,
            "rocprof_source": lt["source"] if lt else None,
            "rocprof_build_matches": lt_match,
            "frac_rocprof_median": (alg_bytes / (lt["median_us"] * 1e-6) / 8.0e12) if lt else None,
            "traffic": traffic,
            "traffic_source": traffic_src,
            "traffic_build_matches": traffic_match,
            "frac_traffic": (traffic / (dom_avg_ms * 1e-3) / 8.0e12) if (traffic and dom_avg_ms > 0) else None,
            # the whole leapfrog (row pass + O(n) work + launch gaps + the per-draw / per-doubling host round trips of
            # the timed region) against the same line: SURVEY 8d bytes per leapfrog x leapfrogs/s per chain
            "leapfrog_algorithmic_bytes": leap_bytes,
            "leapfrog_frac": leap_bytes * (lps_total / world) / 8.0e12,
        },
    }


def main():
    args = parse()
    if args.cpu_worker is not None:
        return cpu_worker_main(args)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return self_launch(args, sys.argv[1:])
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" in os.environ and args.gpus != world and args.gpus != 1:
        print(f"bench: --gpus {args.gpus} under a launcher with WORLD_SIZE={world}; the launcher's world is what runs", file=sys.stderr)
    return run_rank(args)


if __name__ == "__main__":
    sys.exit(main() or 0)
