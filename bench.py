#!/usr/bin/env python3
"""Headline benchmark (BASELINE.json): p50 reconcile-to-Ready latency + readyReplicas accuracy
at replicas = 1/2/4/8, plus, with ``--full``, the scale-down (config 4) and two-pool (config 5)
numbers.

Timed region — ``--steps K`` steps, each one a replica sweep of one ``Mi355xPool`` on one node:
  for n in {1, 2, 4, 8} ∩ [1, N] (and N itself):
    replicas 0 -> n   (timed: PATCH accepted by the apiserver -> watch sees status.readyReplicas
                       == n and Ready=True at the new observedGeneration; on the way the manager
                       claims n GPUs through the node agent, the agent probes every GPU with the
                       gfx950 HIP kernels — 1 GiB HBM pattern test + bf16 MFMA GEMM, ABFT-checked,
                       all CUs covered — and advertises them through the ROCm device plugin)
    accuracy check    (readyReplicas vs an independent ground truth: amd-smi CLI health incl.
                       uncorrectable ECC since the bench baseline, kubelet PodResources per
                       resource, ledger as cross-check; gpupool/bench/ground_truth.py)
    replicas n -> 0   (release, waited for)
  The amd-smi CLI read (~0.7 s on hardware) happens once per step and is reported separately
  (``ground_truth_ms_per_step``) so ``operator_ms_per_step`` is the control plane's own time.

A plain run (``--gpus N --steps K --warmup W``) does only what the headline needs: set-up, warm-up,
the K timed steps, ``--dump-outputs`` if asked for, and the JSON line (``value``, ``ms_per_step``,
``per_n`` with its accuracy and device evidence). ``--steps`` is the number of timed steps: a plain
run has no wall budget unless ``--budget-s`` sets one. Everything below is measured only with
``--full``, which also adds the diagnostics that take requests of their own (agent / manager
footprint, the agent's counters, the manager's reconcile traces and the latency split from them).

``--dump-outputs DIR`` writes what the timed path returned in its last step — for every point of
the sweep the pool status its caller received at Ready and the ground truth read beside it — as
``DIR/<name>.npy`` (float64; see ``_dump_outputs``). Only computed values are written (replica
counts, device health, probe verdicts and CU census counts), no timings or bandwidths, so two builds
run with the same arguments can be compared output for output.

With ``--full``, after the timed region (not part of ms_per_step):
  * config 4: ``--scale-down-steps`` x (N GPUs each running a pod -> replicas N//2, timed until
    the pool is Ready at N//2 with the victims' pods evicted and the GPUs released);
  * config 5: ``--pool-steps`` x two pools of N//2 created together, timed until both are Ready,
    per-pool ground truth (needs N >= 2);
  * health: fault -> condition latency with detection included — by the agent's 100 ms health
    poll (a silent ECC counter change) and as an event (overlay rewrite -> inotify, the path an
    amdsmi event takes) — and reaction only (forced sample).

``value`` is the p50 reconcile-to-Ready latency at replicas = N (``--gpus``), the largest point of
the sweep; ``per_n`` holds every point, ``slowest_cycle`` the slowest timed cycle and, with
``--full``, ``e2e_breakdown_p50_ms`` / ``claim_pass_span_p50_ms`` the median split of a cycle (and
the same split for the slowest one). With N GPUs visible (real MI355X) the agent uses the
amdsmi backend and the gfx950 HIP probe in per-GPU probe helpers; without GPUs it falls back to the 8-GPU fake fixture
with a simulated probe, and says so in ``data``. The API server is always the in-repo apiserver
simulator (no kube-apiserver/etcd in this environment).

Launch contract (driver): ``python bench.py --gpus N --steps K --warmup W``; for N>1 under
``torch.distributed.run`` every rank joins a gloo process group for the barriers and rank 0
drives the control plane, which manages all GPUs of the node. The bench process loads the native
libraries the run stands on (``_load_native``; a missing one is an error, ``config.native`` names
them) but issues no GPU work itself (the node agent, a child process, owns the GPUs), so there is
no device stream to synchronise around the timed region. With ``--full`` and N > 1 real GPUs,
after the timed region and after the control plane has released every GPU, each rank all-reduces
over its own GPU in a child process (RCCL over xGMI; ``config.rccl_allreduce``: exactness + bus
bandwidth).
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BASELINE_TARGET_S = 30.0  # p50 reconcile-to-Ready < 30 s (no published number)
METRIC = "p50 reconcile-to-Ready latency (s) + readyReplicas accuracy at replicas=1/2/4/8"


def _dist_init():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    return rank, world


def _barrier(world: int) -> None:
    if world > 1:
        import torch.distributed as dist
        dist.barrier()


def _visible_gpus() -> int:
    # device_count() does not initialise HIP on this image (safe before spawning children)
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 0


def _gather_max(world: int, x: float) -> float:
    if world <= 1:
        return x
    import torch
    import torch.distributed as dist
    t = torch.tensor([x], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def _free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _comm_check(rank: int, world: int, backend: str) -> dict | None:
    """Every rank all-reduces over its own GPU in a child process (gpupool/parallel/rccl_check.py:
    RCCL over xGMI, exact result + bus bandwidth), under a time limit so a fabric fault cannot
    hang the bench; rank 0 returns the summary."""
    import subprocess
    import torch.distributed as dist
    port = [_free_port() if rank == 0 else None]
    dist.broadcast_object_list(port, src=0)
    cmd = [sys.executable, "-m", "gpupool.parallel.rccl_check", "--rank", str(rank), "--world",
           str(world), "--local-rank", os.environ.get("LOCAL_RANK", str(rank)), "--master-port",
           str(port[0])]
    if backend == "gloo":
        cmd += ["--backend", "gloo", "--device", "cpu", "--bytes", str(8 << 20), "--iters", "5"]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=150, cwd=ROOT)
        lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
        res = json.loads(lines[-1]) if p.returncode == 0 and lines else \
            {"rank": rank, "error": f"exit {p.returncode}: {p.stderr[-400:]}"}
    except subprocess.TimeoutExpired:
        res = {"rank": rank, "error": "timed out after 150 s"}
    got: list = [None] * world
    dist.all_gather_object(got, res)
    if rank != 0:
        return None
    ok = [g for g in got if g and "error" not in g]
    out = {"backend": backend if backend == "gloo" else "nccl(RCCL)", "world": world,
           "ranks_ok": len(ok), "exact": all(g.get("exact") for g in ok) and len(ok) == world}
    if ok:
        out.update({"bytes": ok[0]["bytes"], "min_busbw_GBps": min(g["busbw_GBps"] for g in ok),
                    "max_ms": max(g["ms"] for g in ok), "device": ok[0].get("device", "cpu")})
    errs = [g for g in got if g and "error" in g]
    if errs:
        out["errors"] = errs[:4]
    return out


def sweep_for(n: int) -> list[int]:
    return sorted({k for k in (1, 2, 4, 8) if k <= n} | {n})


def _err(e: BaseException, phase: str, **kw) -> dict:
    msg = f"{type(e).__name__}: {e}".strip()
    return {"error": msg[:400], "phase": phase, **kw}


def _span_p50(traces: list[dict]) -> dict:
    """Median ms per span name (spans summed within a pass) over reconcile traces, + pass count."""
    per_span: dict[str, list[float]] = {}
    for t in traces:
        per: dict[str, float] = {}
        for sp in t["spans"]:
            per[sp["name"]] = per.get(sp["name"], 0.0) + sp["ms"]
        per["total"] = t["totalMs"]
        for k, v in per.items():
            per_span.setdefault(k, []).append(v)
    out = {k: round(statistics.median(v), 3) for k, v in sorted(per_span.items())}
    out["passes"] = len(traces)
    return out


def _device_evidence(cs: list[dict]) -> dict:
    """Per-N device-level numbers from the timed cycles' pool status: the claim-time probe per GPU
    (the N probes of one claim run concurrently) and, for N >= 2, the xGMI peer ring of each claim
    (every outgoing link's GB/s) and the pair coverage the rotating ring order reached."""
    out: dict = {}
    probe = [x for cy in cs for x in cy.get("probeMs") or [] if x]
    if probe:
        out["probe_ms_p50"] = round(statistics.median(probe), 3)
        out["probe_ms_max"] = round(max(probe), 3)
    links = [x for cy in cs for x in cy.get("xgmiGBps") or []]
    if links:
        out["xgmi_links_measured"] = len(links)
        out["xgmi_link_GBps_min"] = round(min(links), 1)
        out["xgmi_link_GBps_p50"] = round(statistics.median(links), 1)
    pairs = [p for cy in cs for p in cy.get("xgmiPairs") or [] if p and p[1]]
    if pairs and links:
        last = cs[-1].get("xgmiPairs") or []
        out["xgmi_pairs_covered_last"] = [p[0] for p in last]
        out["xgmi_pairs_total"] = max(p[1] for p in pairs)
    return out


def _window(traces: list[dict], t0: float, t1: float) -> list[dict]:
    return [t for t in traces if t0 <= t["start"] <= t1]


def _dump_outputs(path: str, sweep: list[int], cycles: list[dict]) -> list[str]:
    """``--dump-outputs``: the last timed cycle of every sweep point, as float64 ``.npy`` arrays.

    One entry per sweep point (in sweep order):
      sweep_replicas     the replicas asked for;
      ready_replicas     status.readyReplicas of the pool the caller saw Ready (-1: no such cycle);
      ready_condition    1 if that status carries Ready=True;
      status_devices     len(status.devices);
      truth_ready        the independent ground truth read at that instant;
      accurate           1 if the two agreed (what ``readyReplicas_accuracy`` counts).
    One entry per claimed GPU, the sweep points' devices one after another in status order:
      device_healthy     1 if status.devices[i].health is "Healthy";
      device_advertised  1 if the GPU is advertised to the kubelet;
      probe_passed       the claim-time probe's verdict (HBM pattern test, MFMA GEMM + ABFT);
      probe_cus_expected / probe_cus_verified   the CU census: compute units the GPU has and
                         those whose matrix cores proved themselves (-1: census not reported).
    Timings and bandwidths are left out: they are measurements, not results."""
    import numpy as np
    last = {cy["n"]: cy for cy in cycles}  # the latest cycle of each N wins
    per_point: dict[str, list[float]] = {k: [] for k in (
        "sweep_replicas", "ready_replicas", "ready_condition", "status_devices", "truth_ready",
        "accurate")}
    fields = (("probe_passed", "passed"), ("probe_cus_expected", "cusExpected"),
              ("probe_cus_verified", "cusVerified"))
    per_dev: dict[str, list[float]] = {name: [] for name in (
        "device_healthy", "device_advertised", *(f for f, _ in fields))}
    for k in sweep:
        cy = last.get(k)
        st = (cy or {}).get("status") or {}
        per_point["sweep_replicas"].append(k)
        per_point["ready_replicas"].append(st.get("readyReplicas", -1) if cy else -1)
        per_point["ready_condition"].append(int(any(
            c.get("type") == "Ready" and c.get("status") == "True"
            for c in st.get("conditions") or [])))
        per_point["status_devices"].append(len(st.get("devices") or []))
        per_point["truth_ready"].append(((cy or {}).get("truth") or {}).get("ready", -1))
        per_point["accurate"].append(int(bool((cy or {}).get("ok"))))
        for d in st.get("devices") or []:
            per_dev["device_healthy"].append(int(d.get("health") == "Healthy"))
            per_dev["device_advertised"].append(int(bool(d.get("advertised"))))
            for name, key in fields:
                v = (d.get("probe") or {}).get(key)
                per_dev[name].append(-1 if v is None else float(v))
    os.makedirs(path, exist_ok=True)
    for name, vals in {**per_point, **per_dev}.items():
        np.save(os.path.join(path, name + ".npy"), np.asarray(vals, dtype=np.float64))
    return sorted({**per_point, **per_dev})


def _load_native(real: bool) -> dict:
    """Load the native libraries this run stands on into this process, before any child starts,
    and name them in the result: libmi355x_dev.so (both device backends, the health verdicts and
    GPU selection the agent calls) and, on real GPUs, libmi355x_probe.so with its gfx950 kernels.
    A library that is missing or does not load ends the run here with its error — with GPUs
    visible the bench never falls back to the simulated probe — instead of surfacing as a claim
    that times out inside a probe helper. Loading initialises no HIP device in this process: the
    GPU work stays with the agent's helpers."""
    from gpupool.ops import devlib, probe
    out = {"libmi355x_dev": devlib.version()}
    if real:
        probe.lib()
        out["libmi355x_probe"] = "loaded (gfx950 probe kernels; devices initialised by the helpers)"
    return out


def main() -> int:
    t_main = time.monotonic()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--backend", default="auto", choices=["auto", "real", "fake"])
    ap.add_argument("--hbm-bytes", type=int, default=1 << 30,
                    help="probe HBM bytes per GPU (CRD default 1 GiB)")
    ap.add_argument("--workdir", default="")
    ap.add_argument("--keep", action="store_true", help="keep the workdir (logs)")
    ap.add_argument("--timeout", type=float, default=120.0, help="per-transition timeout (s)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the secondary scenarios (scale-down, two "
                         "pools, AzureVmPool, health latency, accuracy under faults, the N>1 "
                         "collective check) and collect the footprint / trace diagnostics")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step returned as DIR/<name>.npy")
    ap.add_argument("--budget-s", type=float, default=0.0,
                    help="wall budget for the whole run (s): work not started by then is skipped "
                         "and reported as such; the JSON line is always printed (default: 480 "
                         "with --full, none for a plain run, so --steps sets the timed steps)")
    ap.add_argument("--sample-interval", type=float, default=1.0,
                    help="agent full-telemetry sample period (s)")
    ap.add_argument("--scale-down-steps", type=int, default=3, help="config 4 repetitions (0 = skip)")
    ap.add_argument("--pool-steps", type=int, default=3, help="config 5 repetitions (0 = skip)")
    ap.add_argument("--azure-steps", type=int, default=3,
                    help="config 1 (AzureVmPool replicas=0 -> Ready) repetitions (0 = skip)")
    ap.add_argument("--health-steps", type=int, default=5,
                    help="fault->condition measurements (0 = skip)")
    ap.add_argument("--fault-steps", type=int, default=20,
                    help="readyReplicas-vs-ground-truth checks after random fault/clear steps "
                         "(accuracy_under_faults; 0 = skip)")
    ap.add_argument("--comm-check", default="auto", choices=["auto", "gloo", "off"],
                    help="after the timed region with N>1 ranks: all-reduce across the ranks' "
                         "GPUs over RCCL (auto: when the GPUs are real) or gloo on CPU")
    ap.add_argument("--probe-mode", default="",
                    choices=["", "helper", "helper-sim", "inproc", "simulated"],
                    help="where the agent runs the claim-time probe (default: helper on real GPUs "
                         "— per-GPU child processes, the production setting — helper-sim on the "
                         "fake backend; inproc only for an A/B of the helper's cost)")
    ap.add_argument("--inject-claim-hang", default="",
                    help="fault injection: COUNT:SECONDS — the agent stalls every claim of >= "
                         "COUNT GPUs (exercises the bench's failure isolation)")
    args = ap.parse_args()
    if not args.full:  # a plain run: the headline only
        args.scale_down_steps = args.pool_steps = args.azure_steps = 0
        args.health_steps = args.fault_steps = 0
        args.comm_check = "off"
    budget_s = args.budget_s or (480.0 if args.full else 0.0)
    deadline = t_main + budget_s if budget_s else 0.0  # 0: no wall budget

    def budget_left() -> float:
        return deadline - time.monotonic() if deadline else float("inf")

    rank, world = _dist_init()
    n = args.gpus
    sweep = sweep_for(n)
    visible = _visible_gpus()
    real = args.backend == "real" or (args.backend == "auto" and visible >= n)
    native = _load_native(real)

    cluster = run = pool = None
    cycles: list[dict] = []
    errors: dict[str, list[dict]] = {}     # per N (str) and per scenario
    skipped: dict[str, str] = {}
    failed_at: int | None = None           # smallest N whose cycle failed: larger N are skipped
    pool_ok = True                         # the bench pool is back at 0 after every failure
    setup_error: dict | None = None
    timed_steps = 0
    if rank == 0:
        from gpupool.bench.runner import BenchRun
        from gpupool.testing.cluster import Cluster, NodeSpec
        workdir = args.workdir or tempfile.mkdtemp(prefix="gpupool-bench-")
        # fake mode: simulated probe latency calibrated to the measured real 1 GiB probe
        # (profiles/r1z_bench_kernel_stats.csv: ~1.0 ms claim-time probe)
        extra = [] if real else ["--probe-sim-ms", "1.0"]
        if args.inject_claim_hang:
            extra += ["--inject-claim-delay", args.inject_claim_hang]
        node = NodeSpec("mi355x-node-0", backend="amdsmi" if real else "fake",
                        probe=args.probe_mode or ("helper" if real else "helper-sim"),
                        count=-1 if real else max(8, n), extra_args=extra)
        # production agent settings: ledger fsync on, 100 ms health poll, full sample every 1 s
        cluster = Cluster(workdir, nodes=[node], sample_interval=args.sample_interval, fsync=True)
        try:
            cluster.start()  # all child processes exist before anything touches the GPU
            run = BenchRun(cluster, node, real, hbm_bytes=args.hbm_bytes, timeout=args.timeout,
                           deadline=deadline)
            pool = run.make_pool("bench-pool", "amd.com/gpu", 0)
            run.scale("bench-pool", 0)
            run.refresh_health()  # also fixes the ECC baseline (CLI) for the whole run
        except Exception as e:
            setup_error = _err(e, "setup")
            pool_ok = False

        def failed(k: int, e: BaseException, step: int, stage: str) -> None:
            nonlocal failed_at, pool_ok
            errors.setdefault(str(k), []).append(_err(e, f"{stage}:{run.phase}", step=step))
            failed_at = k if failed_at is None else min(failed_at, k)
            pool_ok = run.recover("bench-pool", min(max(args.timeout, 30.0), budget_left()))
            if not pool_ok:
                errors.setdefault(str(k), []).append(
                    {"error": "pool did not return to 0 replicas", "phase": "recover", "step": step})

        for w in range(args.warmup if pool_ok else 0):
            for k in sweep:
                if not pool_ok or (failed_at is not None and k >= failed_at) or budget_left() <= 0:
                    continue
                try:
                    run.cycle(pool, k)
                except Exception as e:
                    failed(k, e, w, "warmup")
        if run:
            run.gt_s = 0.0
    # the latency clock runs in this process (PATCH sent -> Ready seen on the watch): take the
    # set-up heap (torch, the cluster harness) out of the collector's generations, so a full
    # collection that falls inside a timed cycle costs this process next to nothing
    import gc
    gc.collect()
    gc.freeze()
    _barrier(world)
    footprint_before = run.footprint() if rank == 0 and run and args.full else {}
    t_start = time.perf_counter()
    last_progress = t_start
    # the manager keeps its last 4096 reconcile traces: a long run collects them as it goes (between
    # cycles, outside every cycle's clock) so the slowest cycle's pass is still there at the end
    harvested: dict[str, dict] = {}
    harvest_s = 0.0

    def harvest() -> None:
        nonlocal harvest_s
        t0 = time.perf_counter()
        try:
            for t in cluster.manager_traces(n=2048):
                harvested[str(t.get("reconcileID") or (t.get("key"), t.get("start")))] = t
        except Exception:
            pass
        harvest_s += time.perf_counter() - t0
    if rank == 0 and pool_ok:
        for step in range(args.steps):
            if budget_left() <= 0:
                skipped["timed_steps"] = f"{args.steps - step} of {args.steps} not started: " \
                                         f"wall budget ({budget_s:.0f} s) exhausted"
                break
            try:
                run.refresh_health()
            except Exception as e:
                errors.setdefault("ground_truth", []).append(_err(e, "refresh_health", step=step))
            for k in sweep:
                if failed_at is not None and k >= failed_at:
                    continue
                if budget_left() <= 0:
                    break
                try:
                    cycles.append(run.cycle(pool, k))
                except Exception as e:
                    failed(k, e, step, "timed")
                    if not pool_ok:
                        break
            timed_steps += 1
            if args.full and timed_steps % 100 == 0:
                harvest()
            if time.perf_counter() - last_progress > 20.0:  # a long run shows it is alive
                last_progress = time.perf_counter()
                print(f"# timed step {step + 1}/{args.steps}, {len(cycles)} cycles, "
                      f"{time.perf_counter() - t_start:.0f} s", file=sys.stderr, flush=True)
            if not pool_ok:
                skipped["timed_steps"] = f"{args.steps - step - 1} of {args.steps} not started: " \
                                         "the bench pool could not be recovered"
                break
    _barrier(world)
    elapsed = _gather_max(world, time.perf_counter() - t_start)
    footprint_after = run.footprint() if rank == 0 and run and args.full else {}

    if rank == 0:
        from gpupool.bench.runner import summary
        gt_s = run.gt_s if run else 0.0

        def traces_now() -> list:
            if not args.full:
                return []
            try:
                return cluster.manager_traces(n=2048)
            except Exception:
                return []
        for t in traces_now():
            harvested[str(t.get("reconcileID") or (t.get("key"), t.get("start")))] = t
        traces = sorted((t for t in harvested.values()
                         if t.get("key") in (None, "Mi355xPool/default/bench-pool")),
                        key=lambda t: t.get("start") or 0.0)
        per_n: dict[str, dict] = {}
        for k in sweep:
            cs = [cy for cy in cycles if cy["n"] == k]
            per_n[str(k)] = summary([cy["readySeconds"] for cy in cs], sum(cy["ok"] for cy in cs))
            if cs:  # ground truth read once at Ready (no grace): the fraction of cycles it agreed
                per_n[str(k)]["truth_first_read_agrees"] = round(
                    sum(1 for cy in cs if cy.get("truthFirstReadAgrees")) / len(cs), 4)
                settle = [cy["truth"]["settleMs"] for cy in cs if "settleMs" in cy.get("truth", {})]
                if settle:  # diagnostic: how long the kubelet side lagged when it did not
                    per_n[str(k)]["truth_settle_ms_max"] = max(settle)
                bad = next((cy for cy in cs if not cy.get("ok")), None)
                if bad is not None:  # what the first disagreeing read saw (diagnostic)
                    per_n[str(k)]["first_mismatch"] = {
                        x: bad.get("truth", {}).get(x) for x in (
                            "advertised", "healthyAdvertised", "ready", "ledgerClaimed",
                            "ledgerProbing", "ledgerAgrees", "settleMs", "settled")}
            per_n[str(k)].update(_device_evidence(cs))
            # the agent at this N: its resident memory, the HIP contexts it holds, and the VRAM
            # in use on the GPUs the last cycle of this N claimed (after the timed region)
            fa = (footprint_after or {}).get("agent") or {}
            if "rss_mib" in fa:
                vram = fa.get("vram_used_mib") or {}
                idx = cs[-1].get("indices") or [] if cs else []
                per_n[str(k)]["agent"] = {
                    "rss_mib": fa["rss_mib"], "hip_devices": fa.get("hip_devices"),
                    "vram_used_mib_per_gpu": [vram.get(i) for i in idx]}
                if "helpers_rss_mib" in fa:  # the per-GPU probe helpers beside the agent
                    per_n[str(k)]["agent"].update(probe_helpers=fa.get("helpers"),
                                                  helpers_rss_mib=fa["helpers_rss_mib"],
                                                  helpers_pss_mib=fa.get("helpers_pss_mib"))
                if "fabric_warm" in fa:  # every GPU pair's peer access, before any claim
                    per_n[str(k)]["agent"]["fabric_warm"] = fa["fabric_warm"]
            if str(k) in errors:
                per_n[str(k)]["errors"] = errors[str(k)]
                first = errors[str(k)][0]
                per_n[str(k)].update({"error": first["error"], "phase": first["phase"]})
            elif not cs:
                per_n[str(k)]["skipped"] = (f"N={failed_at} failed earlier" if failed_at is not None
                                            and k > failed_at else skipped.get("timed_steps")
                                            or ("setup failed" if setup_error else "not run"))
        secondary: dict = {}

        def scenario(name: str, reps: int, fn, needs_pool: bool = True):
            """Run ``fn(i)`` reps times, isolated: an exception is recorded with its phase and the
            remaining reps are skipped; the bench pool is brought back to 0 before going on."""
            nonlocal pool_ok
            if reps <= 0:
                return None
            if setup_error is not None:
                secondary[name] = {"skipped": "setup failed"}
                return None
            if needs_pool and not pool_ok:
                secondary[name] = {"skipped": "the bench pool could not be recovered"}
                return None
            out, t0w = [], time.time()
            for i in range(reps):
                if budget_left() <= 0:
                    secondary.setdefault(name, {})["skipped_steps"] = \
                        f"{reps - i} of {reps}: wall budget exhausted"
                    break
                try:
                    out.append(fn(i))
                except Exception as e:
                    secondary.setdefault(name, {})["error"] = _err(e, run.phase, step=i)
                    pool_ok = run.cleanup(pool, name, i, min(max(args.timeout, 30.0), max(1.0, budget_left())))
                    break
            secondary.setdefault(name, {})["_window"] = (t0w, time.time())
            return out

        if pool_ok and n >= 1:
            sd = scenario("scale_down", args.scale_down_steps, lambda i: run.scale_down(pool, n, i))
            if sd:
                secondary["scale_down"].update({
                    **summary([x["seconds"] for x in sd], sum(x["ok"] for x in sd)),
                    "from": n, "to": n // 2, "evicted_per_step": [x["evicted"] for x in sd],
                    "helpers_parked_per_step": [x.get("helpersParked") for x in sd],
                    "helpers_restarting_at_release": [x.get("helpersRestartingAtRelease")
                                                      for x in sd],
                    "claim_helper_waits": [x.get("claimHelperWaits") for x in sd],
                    "claim_helper_wait_ms": [x.get("claimHelperWaitMs") for x in sd],
                    "pods_left_on_released_gpus": sum(len(x["podsOnReleasedGPUs"]) for x in sd)})
        elif args.scale_down_steps > 0:
            secondary["scale_down"] = {"skipped": "the bench pool could not be recovered"
                                       if setup_error is None else "setup failed"}
        if args.pool_steps > 0 and n >= 2:
            tp = scenario("two_pools", args.pool_steps, lambda i: run.two_pools(n, i),
                          needs_pool=False)
            if tp:
                secondary["two_pools"].update({
                    **summary([x["seconds"] for x in tp], sum(x["ok"] for x in tp)),
                    "pools": [n // 2, n // 2],
                    "cross_pool_devices": sum(x["crossPoolDevices"] for x in tp)})
        elif args.pool_steps > 0:
            secondary["two_pools"] = {"skipped": "needs >= 2 GPUs (two pools of N//2)"}
        az = scenario("azure_config1", args.azure_steps, lambda i: run.azure_pool(i),
                      needs_pool=False)
        if az:
            secondary["azure_config1"].update({
                **summary([x["seconds"] for x in az], sum(x["ok"] for x in az)),
                "delete_p50_s": round(statistics.median(x["deleteSeconds"] for x in az), 4),
                "replicas": 0, "cloud": "in-process fake cloud"})
        health: dict = {}
        if args.health_steps > 0:
            hs = scenario("health", 1, lambda i: run.health(pool, args.health_steps))
            got = secondary.pop("health", {})
            health = hs[0] if hs else {k: v for k, v in got.items() if k != "_window"}
        if args.fault_steps > 0:
            fa = scenario("accuracy_under_faults", 1,
                          lambda i: run.accuracy_under_faults(min(n, 8), args.fault_steps))
            if fa:
                secondary["accuracy_under_faults"].update(fa[0])
        try:
            agent_stats = run.agent_stats() if run and args.full else {}
        except Exception as e:
            agent_stats = {"error": repr(e)}
        try:
            metrics = cluster.manager_metrics() if args.full else ""
        except Exception:
            metrics = ""
        all_traces = traces_now()
        # pass-span breakdown of each secondary scenario (scale-down passes, two-pool claims)
        scen_traces = {}
        for name, v in secondary.items():
            w = v.pop("_window", None) if isinstance(v, dict) else None
            if w:
                tr = _window(all_traces, *w)
                scen_traces[name] = tr
                if tr:
                    v["pass_span_p50_ms"] = _span_p50(tr)
        cluster.stop()
        # latency breakdown of the scale-up passes (the reconcile that claims): per timed cycle,
        # the first claiming pass between its PATCH and its Ready
        claim_traces = [t for t in traces
                        if any(sp["name"] == "agent:POST /v1/claims" for sp in t["spans"])]
        e2e: dict[str, list[float]] = {"patch_rtt_ms": [], "patch_to_pass_ms": [],
                                       "queue_wait_ms": [], "pass_ms": [],
                                       "status_to_client_ms": []}
        by_n: dict[int, list[dict]] = {}
        matched: dict[int, dict] = {}  # id(cycle) -> its claiming pass
        for cy in cycles:
            # the claiming pass may have started just before the PATCH landed (a pass already
            # running reads the pool afresh and sees the new replicas): match by overlap
            hit = [t for t in claim_traces if t["start"] <= cy["readyAtWall"]
                   and t["start"] + t["totalMs"] / 1e3 >= cy["patchAt"]]
            if not hit:
                continue
            t = min(hit, key=lambda x: x["start"])
            matched[id(cy)] = t
            by_n.setdefault(cy["n"], []).append(t)
            e2e["patch_to_pass_ms"].append((t["start"] - cy["patchAt"]) * 1e3)
            if cy.get("patchRttMs") is not None:  # the client's PATCH request -> response
                e2e["patch_rtt_ms"].append(cy["patchRttMs"])
            qw = (t.get("attrs") or {}).get("queueWaitMs")
            if qw is not None:  # of which: ready in the manager's work queue, no worker yet
                e2e["queue_wait_ms"].append(float(qw))
            e2e["pass_ms"].append(t["totalMs"])
            e2e["status_to_client_ms"].append(
                (cy["readyAtWall"] - t["start"]) * 1e3 - t["totalMs"])
        span_per_n = {str(k): _span_p50(v) for k, v in sorted(by_n.items())}
        # where the slowest timed cycle's time went (an outlier's cause is otherwise invisible in
        # the medians): its client-side latency split and its claiming pass's spans
        slowest = None
        if cycles:
            cy = max(cycles, key=lambda x: x["readySeconds"])
            slowest = {"n": cy["n"], "ready_ms": round(cy["readySeconds"] * 1e3, 3),
                       "patch_rtt_ms": round(cy.get("patchRttMs") or 0.0, 3),
                       "probe_ms": cy.get("probeMs")}
            t = matched.get(id(cy))
            if t is not None:
                per: dict[str, float] = {}
                for sp in t["spans"]:
                    per[sp["name"]] = round(per.get(sp["name"], 0.0) + sp["ms"], 3)
                slowest.update({
                    "patch_to_pass_ms": round((t["start"] - cy["patchAt"]) * 1e3, 3),
                    "queue_wait_ms": (t.get("attrs") or {}).get("queueWaitMs"),
                    "pass_ms": round(t["totalMs"], 3),
                    "status_to_client_ms": round((cy["readyAtWall"] - t["start"]) * 1e3
                                                 - t["totalMs"], 3),
                    "pass_spans_ms": per})
        e2e_p50 = {k2: round(statistics.median(v), 3) for k2, v in e2e.items() if v}
        e2e_p50["cycles_matched"] = len(e2e["pass_ms"])
        done = [k for k in sweep if per_n[str(k)]["p50_s"] is not None]
        value_n = max(done) if done else None
        head = per_n[str(value_n)] if value_n is not None else {"p50_s": None, "p90_s": None,
                                                               "max_s": None}
        all_ok = sum(cy["ok"] for cy in cycles)
        pmode = args.probe_mode or ("helper" if real else "helper-sim")
        src = ("real MI355X: amdsmi discovery + gfx950 HIP probe (HBM %d MiB + bf16 MFMA, probe "
               "mode %s) + device plugin -> fake kubelet" % (args.hbm_bytes >> 20, pmode)) if real \
            else ("synthetic: 8x MI355X fake fixture (no GPU visible), simulated probe (probe mode "
                  "%s), device plugin -> fake kubelet" % pmode)
        status = "ok" if value_n == n and not errors and not skipped and setup_error is None \
            else "partial" if value_n is not None else "failed"
        out = {
            "metric": METRIC,
            "value": head["p50_s"],
            "unit": "s",
            "n_gpus": n,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed * 1e3 / max(1, timed_steps), 2),
            "higher_is_better": False,
            "scaling": "weak",
            "vs_baseline": round(head["p50_s"] / BASELINE_TARGET_S, 5)
            if head["p50_s"] is not None else None,
            "dtype": "bf16",
            "data": src + "; control plane against the in-repo apiserver-sim (no kube-apiserver/etcd)",
            "status": status,
            "value_n": value_n,
            "config": {
                "model": "Mi355xPool scale 0->n, n in %s (BASELINE configs 2/3/4/5; config 1 in "
                         "azure_config1)" % sweep,
                "global_batch": n,
                "seq_len": 0,
                "parallelism": f"replicas{n}",
                "backend": "amdsmi+hip" if real else "fake",
                "dtype_note": "bf16 = the probe's MFMA GEMM check; the metric is a control-plane latency",
                "baseline_target_s": BASELINE_TARGET_S,
                "value_note": "p50 at replicas=%s (%s)" % (
                    value_n, "the requested N" if value_n == n else
                    "the largest N that completed; see per_n for the failure"),
                "p90_s": head["p90_s"],
                "max_s": head["max_s"],
                "readyReplicas_accuracy": all_ok / len(cycles) if cycles else None,
                # the truth behind that accuracy is read once, at the instant the pool reads Ready
                "truth_first_read_agrees": (round(sum(1 for cy in cycles if cy.get(
                    "truthFirstReadAgrees")) / len(cycles), 4) if cycles else None),
                "readiness_mode": "advertise-on-submit" if os.environ.get(
                    "GPUPOOL_ADVERTISE_ON_SUBMIT") == "1" else "strict (after the ListAndWatch write)",
                "per_n": per_n,
                "timed_steps_completed": timed_steps,
                "operator_ms_per_step": round((elapsed - gt_s - harvest_s) * 1e3 / max(1, timed_steps), 2),
                "trace_harvest_s": round(harvest_s, 3),
                "ground_truth_ms_per_step": round(gt_s * 1e3 / max(1, timed_steps), 2),
                **secondary,
                "health_condition_latency": health,
                "sample_interval_s": args.sample_interval,
                "health_poll_interval_s": 0.1,
                "agent": agent_stats,
                # agent + manager resident memory / threads / fds around the timed region
                "footprint": {"before_timed": footprint_before, "after_timed": footprint_after},
                "world_size": world,
                "claim_pass_span_p50_ms": span_per_n.get(str(value_n), {}),
                "claim_pass_span_p50_ms_per_n": span_per_n,
                "e2e_breakdown_p50_ms": e2e_p50,
                "slowest_cycle": slowest,
                "budget": {"budget_s": budget_s,
                           "used_s": round(time.monotonic() - t_main, 2),
                           "skipped": skipped},
                "steps_detail": [{k2: (round(v, 4) if isinstance(v, float) else v)
                                  for k2, v in cy.items()
                                  if k2 not in ("patchAt", "readyAtWall", "status")}
                                 for cy in cycles[:len(sweep)]],
            },
        }
        out["config"]["full"] = args.full
        out["config"]["native"] = native
        if not args.full:  # what only --full collects is left out, not reported empty
            for k in ("health_condition_latency", "agent", "footprint", "claim_pass_span_p50_ms",
                      "claim_pass_span_p50_ms_per_n", "e2e_breakdown_p50_ms", "trace_harvest_s"):
                out["config"].pop(k, None)
        if args.dump_outputs:
            out["config"]["dumped_outputs"] = _dump_outputs(args.dump_outputs, sweep, cycles)
        if setup_error is not None:
            out["config"]["setup_error"] = setup_error
        for k in ("ground_truth",):
            if k in errors:
                out["config"]["ground_truth_errors"] = errors[k]
    comm_backend = "gloo" if args.comm_check == "gloo" else "nccl" if real else ""
    if world > 1 and args.comm_check != "off" and comm_backend:
        comm = _comm_check(rank, world, comm_backend)
        if rank == 0:
            out["config"]["rccl_allreduce"] = comm
    if rank == 0:
        print(json.dumps(out), flush=True)
        if not args.keep and not args.workdir:
            shutil.rmtree(cluster.workdir, ignore_errors=True)
        else:
            print(f"# workdir kept: {cluster.workdir}", file=sys.stderr)
            with open(os.path.join(cluster.workdir, "manager_metrics.txt"), "w") as f:
                f.write(metrics)
            with open(os.path.join(cluster.workdir, "traces.json"), "w") as f:
                json.dump(traces, f, indent=1)
            for name, tr in scen_traces.items():
                with open(os.path.join(cluster.workdir, f"traces_{name}.json"), "w") as f:
                    json.dump(tr, f, indent=1)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
