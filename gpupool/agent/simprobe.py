"""Simulated probe kernels for the fake device backend on CPU-only hosts.

The same results the gfx950 kernels report (probe.hip), timed like them, failing only where the
fault overlay says so. Used by the agent's ``simulated`` probe mode (in process) and by the
``helper-sim`` probe helpers (probehost.py), so the helper machinery — child processes, deadlines,
crash handling — is exercised on CPU with the exact results the in-process simulation gives.
"""
from __future__ import annotations

import time

from ..api import schema

# nominal numbers = the measured MI355X probe (profiles/r1c_probe_gemm_ab_real.json)
SIM_HBM_GBPS = 4900.0
SIM_MFMA_TFLOPS = 1200.0
SIM_XGMI_GBPS = 64.0
SIM_SWEEP_GBPS = 6000.0
# the low-precision GEMMs at the claim-time size 2048^3 (profiles/lowp_gemm_rates.json)
# the PCIe host link's slower direction (device -> host) at the default 4 MiB, alone on the GPU
# (profiles/hostlink_rates.json)
SIM_HOSTLINK_GBPS = 51.0
# the LDS phase's grid factor and kernel time (native/src/probe/options.h lds::kBlocksPerCU,
# profiles/lds_claim_probe_cost.json)
SIM_LDS_BLOCKS_PER_CU = 4
SIM_LDS_MS = 0.2
# the register-file phase's grid factor and kernel time (native/src/probe/options.h
# regs::kBlocksPerCU, profiles/regs_claim_probe_cost.json)
SIM_REGS_BLOCKS_PER_CU = 2
SIM_REGS_MS = 0.15
# the vector-ALU phase's grid factor, step count and kernel time (native/src/probe/options.h
# alu::kBlocksPerCU, alu::kIters, profiles/alu_claim_probe_cost.json) and the digest it reports
SIM_ALU_BLOCKS_PER_CU = 1
SIM_ALU_ITERS = 64
SIM_ALU_MS = 0.14
SIM_ALU_TRANS_DIGEST = "0" * 16
# the atomic-unit phase's grid factor, step count, layer mask and kernel time (native/src/probe/options.h
# atom::kBlocksPerCU, atom::kIters, atom::kLayerMask; profiles/atomics_claim_probe_cost.json and _run2.json:
# every CU verified at factor 1 in 400 runs per setting, 2 steps add +0.037 ms to the claim probe in both
# runs, the two kernels take 0.10 ms alone)
SIM_ATOM_BLOCKS_PER_CU = 1
SIM_ATOM_ITERS = 2
SIM_ATOM_LAYERS = 7
SIM_ATOM_MS = 0.1
SIM_LOWP_TFLOPS = {"fp8": 696.0, "mxfp8": 477.0, "mxfp4": 523.0}


def fault(dev: dict, key: str):
    """A fault-overlay key of one device (the overlay merges device keys into the snapshot;
    older fixtures nest them under ``faults``)."""
    v = dev.get(key)
    return v if v is not None else (dev.get("faults") or {}).get(key)


def _verified_per_xcd(cus: int, bad: int) -> list:
    """``cus`` CUs spread over the 8 XCDs, less ``bad`` taken from the front, XCD by XCD."""
    per = [cus // 8 + (1 if x < cus % 8 else 0) for x in range(8)]
    for x in range(8):
        take = min(bad, per[x])
        per[x] -= take
        bad -= take
    return per


def probe(dev: dict, opts: dict, sim_ms: float) -> dict:
    t0 = time.perf_counter()
    hbm = int(opts.get("hbmBytes", 1 << 30))
    mfma = bool(opts.get("mfma", True))
    time.sleep(sim_ms / 1e3)
    fail = bool(fault(dev, "probeFail"))
    res = {"passed": not fail, "backend": "simulated",
           "hbm": {"ok": not fail, "GBps": SIM_HBM_GBPS, "bytes": hbm},
           "mfma": {"ok": not fail, "tflops": SIM_MFMA_TFLOPS if mfma else 0.0, "enabled": mfma}}
    if mfma:  # the CU census: every CU of this (partition of the) GPU proves its MFMA pipes
        cus = int((dev.get("asic") or {}).get("computeUnits") or 256)
        dead = int(dev.get("cuFault") or 0)
        res["cus"] = {"expected": cus, "mfmaVerified": cus - dead, "badWaves": dead * 8,
                      "ok": dead == 0}
        if dead and not fail:
            res["passed"] = False
        # spec.probe.mfmaLowPrecision: the same block the gfx950 probe reports; the overlay's
        # ``lowpFault: "<dtype>"`` fails that dtype's ABFT check only
        asked = list(opts.get("mfmaLowPrecision") or [])
        if asked:
            bad = fault(dev, "lowpFault")
            res["lowp"] = {d: {"ok": d != bad, "n": 2048, "elementMismatches": 0,
                               "abftMismatches": 2 if d == bad else 0,
                               "tflops": SIM_LOWP_TFLOPS.get(d, 0.0), "ms": 0.05,
                               "cusVerified": cus - dead, "badWaves": dead * 8} for d in asked}
            if bad in asked:
                res["passed"] = False
    # spec.probe.hostLinkCheck: the block the gfx950 probe reports; the overlay's ``hostLinkFail``
    # flips one bit on that GPU's link
    if opts.get("hostLinkCheck"):
        bad = bool(fault(dev, "hostLinkFail"))
        nbytes = int(opts.get("hostLinkBytes") or schema.DEFAULT_HOST_LINK_BYTES)
        res["hostLink"] = {"ok": not bad, "bytes": nbytes, "patterns": 2,
                           "seed": 0x4C4B0000 + int(dev.get("index") or 0),
                           "badBits": 1 if bad else 0, "firstBadOffset": 0 if bad else None,
                           "hostSamples": 1026, "hostSampleMismatches": 0,
                           "writeGBps": SIM_HOSTLINK_GBPS, "readGBps": SIM_HOSTLINK_GBPS,
                           "GBps": SIM_HOSTLINK_GBPS, "ms": 4 * nbytes / (SIM_HOSTLINK_GBPS * 1e6),
                           "allocMs": 0.0}
        if bad:
            res["passed"] = False
    # spec.probe.ldsCheck: the block the gfx950 probe reports; the overlay's ``ldsFault: n`` marks n
    # CUs bad, one flipped bit each, the first on the CU with key 0 at LDS offset 0
    if opts.get("ldsCheck"):
        cus = int((dev.get("asic") or {}).get("computeUnits") or 256)
        bad = min(cus, int(fault(dev, "ldsFault") or 0))
        per = _verified_per_xcd(cus, bad)
        res["lds"] = {"ok": bad == 0, "bytesPerCU": 163840, "patterns": 2, "salt": 0,
                      "workgroups": SIM_LDS_BLOCKS_PER_CU * cus, "cusTested": cus,
                      "cusVerified": cus - bad, "perXcd": per, "badCUs": bad, "badBits": bad,
                      "firstBadCU": 0 if bad else None, "firstBadOffset": 0 if bad else None,
                      "ms": SIM_LDS_MS}
        if bad:
            res["passed"] = False
    # spec.probe.registerCheck: the block the gfx950 probe reports; the overlay's ``regFault: n``
    # marks n CUs bad, one flipped bit each, the first on the CU with key 0, SIMD 0, register v17, lane 0
    if opts.get("registerCheck"):
        cus = int((dev.get("asic") or {}).get("computeUnits") or 256)
        bad = min(cus, int(fault(dev, "regFault") or 0))
        per = _verified_per_xcd(cus, bad)
        res["regs"] = {"ok": bad == 0, "registersPerLane": 512, "workgroupsPerCU": 1, "patterns": 2,
                       "salt": 0, "workgroups": SIM_REGS_BLOCKS_PER_CU * cus, "cusTested": cus,
                       "cusVerified": cus - bad, "simdsTested": 4 * cus, "simdShort": 0, "perXcd": per,
                       "badCUs": bad, "badBits": bad, "firstBadCU": 0 if bad else None,
                       "firstBadSimd": 0 if bad else None, "firstBadRegister": 17 if bad else None,
                       "firstBadLane": 0 if bad else None, "ms": SIM_REGS_MS}
        if bad:
            res["passed"] = False
    # spec.probe.aluCheck: the block the gfx950 probe reports; the overlay's ``aluFault: n`` marks n CUs
    # bad, every wave on them with one lane off the host's digest, the first on the CU with key 0,
    # SIMD 0, group f32, lane 0
    if opts.get("aluCheck"):
        cus = int((dev.get("asic") or {}).get("computeUnits") or 256)
        bad = min(cus, int(fault(dev, "aluFault") or 0))
        per = [4 * n for n in _verified_per_xcd(cus, bad)]  # SIMDs
        wg = SIM_ALU_BLOCKS_PER_CU * cus
        res["alu"] = {"ok": bad == 0, "iters": SIM_ALU_ITERS, "workgroups": wg, "waves": 4 * wg,
                      "wavesPerSimd": [wg] * 4, "simdsTested": 4 * cus, "simdsVerified": 4 * (cus - bad),
                      "cusVerified": cus - bad, "perXcd": per, "badWaves": 4 * SIM_ALU_BLOCKS_PER_CU * bad,
                      "badLanes": 4 * SIM_ALU_BLOCKS_PER_CU * bad, "badCUs": bad,
                      "firstBadCU": 0 if bad else None, "firstBadSimd": 0 if bad else None,
                      "firstBadGroup": "f32" if bad else None, "firstBadLane": 0 if bad else None,
                      "splitWaves": 0, "suspectCU": None, "suspectSimd": None,
                      "transDigest": SIM_ALU_TRANS_DIGEST, "ms": SIM_ALU_MS}
        if bad:
            res["passed"] = False
    # spec.probe.atomicsCheck: the block the gfx950 probe reports; the overlay's ``atomicsFault: n`` marks
    # n CUs bad, the workgroup on each with one slot of the LDS table off the host's value, the first
    # on the CU with key 0, op add, slot 0
    if opts.get("atomicsCheck"):
        cus = int((dev.get("asic") or {}).get("computeUnits") or 256)
        bad = min(cus, int(fault(dev, "atomicsFault") or 0))
        full, per = _verified_per_xcd(cus, 0), _verified_per_xcd(cus, bad)
        wg = SIM_ATOM_BLOCKS_PER_CU * cus
        res["atomics"] = {"ok": bad == 0, "iters": SIM_ATOM_ITERS, "layers": SIM_ATOM_LAYERS, "workgroups": wg,
                          "wgPerXcd": [SIM_ATOM_BLOCKS_PER_CU * n for n in full], "cusTested": cus,
                          "cusVerified": cus - bad, "perXcd": per, "badCUs": bad,
                          "badWorkgroups": SIM_ATOM_BLOCKS_PER_CU * bad, "ldsBadSlots": SIM_ATOM_BLOCKS_PER_CU * bad,
                          "l2BadSlots": 0, "devBadSlots": 0, "badReturns": 0, "ticketFaults": 0,
                          "firstBadCU": 0 if bad else None, "firstBadLayer": "lds" if bad else None,
                          "firstBadOp": "add" if bad else None, "firstBadSlot": 0 if bad else None,
                          "firstBadXcc": 0 if bad else None, "ms": SIM_ATOM_MS}
        if bad:
            res["passed"] = False
    if fail:
        res["error"] = "injected probe failure (fault overlay)"
    res["ms"] = (time.perf_counter() - t0) * 1e3
    return res


def sweep_window(dev: dict, offset: int, window: int, reserve: int) -> dict:
    """One HBM scrub window: nominal timing of the real kernels (~6 TB/s over 4 passes); flipped
    bits where the overlay's ``hbmBadOffset`` (a byte offset) falls inside the window."""
    span = max(window, int(dev.get("memTotalBytes") or 288e9) - reserve)
    off = offset % span
    n = min(window, span - off)
    time.sleep(min(0.05, 4 * n / 6e12))
    bad_at = fault(dev, "hbmBadOffset")
    bad = 1 if bad_at is not None and off <= int(bad_at) < off + n else 0
    return {"passed": not bad, "offset": off, "bytes": n, "span": span, "badBits": bad,
            "firstBadOffset": int(bad_at) if bad else None, "GBps": SIM_SWEEP_GBPS, "ms": 0.0}


def link(src: dict, dst: dict) -> dict:
    """One simulated xGMI peer copy src -> dst (overlay: xgmiPeerFail, xgmiBadPeers [indices],
    xgmiPeerUnavailable, probeScale)."""
    faults = {**(src.get("faults") or {}), **src}
    bad = bool(faults.get("xgmiPeerFail")) or dst.get("index") in (faults.get("xgmiBadPeers") or [])
    if faults.get("xgmiPeerUnavailable"):
        return {"passed": False, "canAccessPeer": False, "error": "hipDeviceCanAccessPeer=0"}
    r = {"passed": not bad, "canAccessPeer": True,
         "GBps": SIM_XGMI_GBPS * float(faults.get("probeScale") or 1.0), "badBits": 0 if not bad else 1}
    if bad:
        r["error"] = "injected xGMI peer failure (fault overlay)"
    return r
