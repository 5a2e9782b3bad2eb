"""ctypes binding for libmi355x_probe.so — the gfx950 HIP readiness probe (probe.hip).

``init()`` warms every HIP context once (done by the long-lived node agent at start-up), so a
claim-time ``run()`` pays only its kernels. ``run()`` releases the GIL (ctypes does), so probes of
different GPUs run concurrently from a thread pool.
"""
from __future__ import annotations

import ctypes
import functools
import json
import threading

from . import lowp, native_path
from .probe_checks import CHECKS

_lib = None
_lock = threading.Lock()
_count: int | None = None


def lib() -> ctypes.CDLL:
    global _lib
    with _lock:
        if _lib is None:
            l = ctypes.CDLL(native_path("libmi355x_probe.so"))
            l.mi355x_probe_init.restype = ctypes.c_int
            l.mi355x_probe_init.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
            l.mi355x_probe_device_count.restype = ctypes.c_int
            l.mi355x_probe_identify.restype = ctypes.c_void_p
            l.mi355x_probe_identify.argtypes = [ctypes.c_int]
            l.mi355x_probe_run.restype = ctypes.c_void_p
            l.mi355x_probe_run.argtypes = [ctypes.c_int, ctypes.c_char_p]
            l.mi355x_probe_free.argtypes = [ctypes.c_void_p]
            l.mi355x_probe_peer.restype = ctypes.c_void_p
            l.mi355x_probe_peer.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
            if hasattr(l, "mi355x_probe_peer_dump"):  # absent from a library built before it
                l.mi355x_probe_peer_dump.restype = ctypes.c_void_p
                l.mi355x_probe_peer_dump.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                                     ctypes.c_void_p, ctypes.c_size_t]
            if hasattr(l, "mi355x_probe_peer_ring"):  # absent from a library built before it
                l.mi355x_probe_peer_ring.restype = ctypes.c_void_p
                l.mi355x_probe_peer_ring.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                                     ctypes.c_char_p]
            l.mi355x_probe_trim.restype = ctypes.c_int
            l.mi355x_probe_trim.argtypes = [ctypes.c_int]
            l.mi355x_probe_hbm_sweep.restype = ctypes.c_void_p
            l.mi355x_probe_hbm_sweep.argtypes = [ctypes.c_int, ctypes.c_char_p]
            l.mi355x_probe_sweep_alloc.restype = ctypes.c_int
            l.mi355x_probe_sweep_alloc.argtypes = [ctypes.c_int, ctypes.c_longlong]
            l.mi355x_probe_sweep_release.restype = ctypes.c_int
            l.mi355x_probe_sweep_release.argtypes = [ctypes.c_int]
            l.mi355x_probe_gemm_bf16.restype = ctypes.c_int
            l.mi355x_probe_gemm_bf16.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int]
            if hasattr(l, "mi355x_probe_gemm_bf16_opts"):  # absent from a library built before it
                l.mi355x_probe_gemm_bf16_opts.restype = ctypes.c_int
                l.mi355x_probe_gemm_bf16_opts.argtypes = [ctypes.c_int, ctypes.c_void_p,
                                                          ctypes.c_void_p, ctypes.c_void_p,
                                                          ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                          ctypes.c_char_p]
            if hasattr(l, "mi355x_probe_gemm_lowp"):  # absent from a library built before it
                l.mi355x_probe_gemm_lowp.restype = ctypes.c_int
                l.mi355x_probe_gemm_lowp.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 5 + \
                    [ctypes.c_int] * 3 + [ctypes.c_char_p]
            if hasattr(l, "mi355x_probe_host_link"):  # absent from a library built before it
                l.mi355x_probe_host_link.restype = ctypes.c_void_p
                l.mi355x_probe_host_link.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p,
                                                     ctypes.c_size_t]
                l.mi355x_probe_host_link_geometry.restype = None
                l.mi355x_probe_host_link_geometry.argtypes = [ctypes.POINTER(ctypes.c_int)] * 3
            if hasattr(l, "mi355x_probe_lds"):  # absent from a library built before it
                l.mi355x_probe_lds.restype = ctypes.c_void_p
                l.mi355x_probe_lds.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t]
            if hasattr(l, "mi355x_probe_regs"):  # absent from a library built before it
                l.mi355x_probe_regs.restype = ctypes.c_void_p
                l.mi355x_probe_regs.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t]
            if hasattr(l, "mi355x_probe_alu"):  # absent from a library built before it
                l.mi355x_probe_alu.restype = ctypes.c_void_p
                l.mi355x_probe_alu.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t]
            if hasattr(l, "mi355x_probe_atomics"):  # absent from a library built before it
                l.mi355x_probe_atomics.restype = ctypes.c_void_p
                l.mi355x_probe_atomics.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_size_t]
            if hasattr(l, "mi355x_probe_abft_check"):  # absent from a library built before them
                vp, ull = ctypes.c_void_p, ctypes.c_ulonglong
                l.mi355x_probe_abft_check.restype = ctypes.c_int
                l.mi355x_probe_abft_check.argtypes = [ctypes.c_int, ctypes.c_int] + [vp] * 5 + \
                    [ctypes.c_int] * 3 + [ctypes.c_float, vp, vp, ctypes.c_int, vp, vp, vp]
                l.mi355x_probe_gemm_ref.restype = ctypes.c_int
                l.mi355x_probe_gemm_ref.argtypes = [ctypes.c_int, ctypes.c_int] + [vp] * 5 + [ctypes.c_int] * 3
                l.mi355x_probe_count_diff.restype = ctypes.c_int
                l.mi355x_probe_count_diff.argtypes = [ctypes.c_int, vp, vp, ull, ctypes.POINTER(ull)]
                l.mi355x_probe_gen_operands.restype = ctypes.c_int
                l.mi355x_probe_gen_operands.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_int,
                                                        ull, ull, vp, ctypes.c_size_t, vp, ctypes.c_size_t,
                                                        vp, ctypes.c_size_t]
            _lib = l
    return _lib


def _take(p) -> dict:
    if not p:
        raise RuntimeError("libmi355x_probe returned NULL")
    try:
        return json.loads(ctypes.string_at(p).decode())
    finally:
        lib().mi355x_probe_free(p)


def init() -> int:
    """Initialise HIP + warm all visible devices. Returns the HIP device count."""
    global _count
    if _count is not None:
        return _count
    err = ctypes.create_string_buffer(512)
    n = lib().mi355x_probe_init(err, len(err))
    if n < 0:
        raise RuntimeError(f"HIP probe init failed: {err.value.decode()}")
    _count = n
    return n


def identify(dev: int) -> dict:
    return _take(lib().mi355x_probe_identify(dev))


def run(dev: int, hbm_bytes: int = 1 << 30, mfma: bool = True, gemm_n: int = 4096,
        patterns: int = 2, gemm_reps: int = 1, gemm_tile: int = 256, mfma_low_precision=(),
        host_link_bytes: int = 0, lds_check: bool = False, reg_check: bool = False,
        alu_check: bool = False, atom_check: bool = False, **test_hooks: int) -> dict:
    """Probe HIP device ``dev``. ``gemm_tile`` 256 (default, the glds 256x256 kernel) or 128 (the
    older register-staged kernel, for A/B). ``mfma_low_precision``: names out of ``lowp.DTYPES``
    ("fp8", "mxfp8", "mxfp4"); each adds a census, a 256^3 GEMM against a VALU reference and the
    gemm_n GEMM with ABFT on that dtype's matrix-core instruction, reported under "lowp" (needs
    ``mfma``). ``host_link_bytes`` > 0 adds the PCIe host-link phase over that many bytes of pinned
    host memory (written and read back by the GPU over the link, every bit verified, both
    directions timed), reported under "hostLink". ``lds_check`` adds the per-CU LDS phase (every
    CU's 160 KiB marched in both polarities and address-tested by a workgroup that owns it),
    reported under "lds"; its knobs and hooks (ldsBytes, ldsPatterns, ldsSalt, ldsBlocksPerCU,
    ldsFirst, injectLdsFlipAtByte, injectLdsFaultXcc, injectLdsSkipChunk) go with the test hooks.
    ``reg_check`` adds the register-file phase (all 512 vector registers of every lane of every SIMD
    of every CU marched in both polarities by a workgroup that owns the CU), reported under "regs";
    its knobs and hooks (regsPatterns, regsSalt, regsBlocksPerCU, regsFirst, injectRegFlip=[u, lane,
    bit], injectRegFaultSimd, injectRegFaultXcc, injectRegSkip) go with the test hooks too.
    ``alu_check`` adds the vector-ALU phase (a fixed program of integer, f32, f64, packed-f16, cross-lane
    and transcendental instructions on every SIMD of every CU, each lane's digests compared with the
    host's, the transcendental ones with the device's consensus), reported under "alu"; its knobs and
    hooks (aluIters, aluBlocksPerCU, aluFirst, aluSeed, injectAluFlip=[group, step, lane, bit],
    injectAluFaultSimd, injectAluFaultXcc) go with the test hooks too.
    ``atom_check`` adds the atomic-unit phase (a fixed program of atomic read-modify-write instructions
    through every CU's LDS atomic unit, through the L2 atomic units and at device scope across the XCDs,
    every final and returned value compared with the host's), reported under "atomics"; its knobs and
    hooks (atomIters, atomBlocksPerCU, atomLayers, atomFirst, atomSeed, injectAtomSkip=[layer, op, step,
    lane], injectAtomFlip=[layer, op, step, lane, bit], injectAtomFaultXcc, injectAtomFaultWorkgroup) go
    with the test hooks too.
    ``test_hooks``: injectBitFlips=N (N bits spread over
    the HBM region) / injectFlipAtChunk=i (bit 0 of 16-byte chunk i) / injectGemmFault=1 corrupt
    the device buffers between compute and check so tests can prove the checkers catch faults;
    injectGemmFaultRow / injectGemmFaultCol place the GEMM fault (and injectLowpFault's) at that
    element of C instead of row gemm_n/3, column gemm_n/5 — outside C: no fault."""
    opts = _run_opts(int(hbm_bytes), bool(mfma), int(gemm_n), int(patterns), int(gemm_reps),
                     int(gemm_tile), tuple(sorted((k, _hook(v)) for k, v in test_hooks.items())),
                     tuple(mfma_low_precision), int(host_link_bytes), bool(lds_check), bool(reg_check),
                     **{k: True for k, on in (("alu_check", alu_check), ("atom_check", atom_check)) if on})
    return _take(lib().mi355x_probe_run(dev, opts))


def _hook(v):
    """A hook's value: an integer, or a tuple of them (injectRegFlip)."""
    return tuple(int(x) for x in v) if isinstance(v, (list, tuple)) else int(v)


@functools.lru_cache(maxsize=64)
def _run_opts(hbm_bytes: int, mfma: bool, gemm_n: int, patterns: int, gemm_reps: int,
              gemm_tile: int, hooks: tuple, low_precision: tuple = (),
              host_link_bytes: int = 0, lds_check: bool = False, reg_check: bool = False,
              alu_check: bool = False, atom_check: bool = False) -> bytes:
    # An agent probes with a handful of option sets: encode each once. Encoding it per claim cost
    # 0.05 ms on a CPU woken from idle (profiles/r4n_probe_idle_binding.json).
    opts = {"hbmBytes": hbm_bytes, "mfma": mfma, "gemmN": gemm_n, "patterns": patterns,
            "gemmReps": gemm_reps, "gemmTile": gemm_tile, **dict(hooks)}
    if low_precision:  # the library's option parser reads integers: a dtype bit mask
        opts["mfmaLowPrecision"] = lowp.dtype_mask(low_precision)
    if host_link_bytes > 0:  # absent when off: the default options stay what they were
        opts["hostLinkBytes"] = host_link_bytes
    for check, on in zip(CHECKS, (lds_check, reg_check, alu_check, atom_check)):
        if on:  # absent when off, likewise
            opts[check.option] = 1
    return json.dumps(opts).encode()


def host_link_geometry() -> dict:
    """The default launch shape of the host-link kernels {"grid", "threads", "unroll"}: one pass of
    the main loop of the whole grid covers grid * threads * unroll 16-byte chunks."""
    if not hasattr(lib(), "mi355x_probe_host_link"):
        raise RuntimeError("libmi355x_probe.so predates the host-link check: rebuild it")
    g, t, u = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib().mi355x_probe_host_link_geometry(ctypes.byref(g), ctypes.byref(t), ctypes.byref(u))
    return {"grid": g.value, "threads": t.value, "unroll": u.value}


def host_link(dev: int, nbytes: int, patterns: int = 2, preload=None, want_bytes: int = 0,
              **hooks: int) -> dict:
    """The host-link phase alone (``mi355x_probe_host_link``): ``nbytes // 16`` chunks of pinned
    host memory written by the GPU over PCIe, read back and verified, ``patterns`` passes. ->
    the "hostLink" block of ``run`` plus "device" and "passed". ``want_bytes`` > 0: the first
    ``min(want_bytes, tested bytes)`` of the pinned buffer after the run come back under "data"
    (bytes). ``preload`` (a bytes-like object or a C-contiguous uint8 numpy array): no write pass;
    the buffer is loaded from it and verified once against polarity 0 over ``len(preload) // 16``
    chunks (``nbytes`` is ignored). ``hooks``: injectHostLinkFlipAtChunk=i and the sweep's knobs
    hostLinkGrid / hostLinkUnroll / hostLinkNT / hostLinkCoherent."""
    if not hasattr(lib(), "mi355x_probe_host_link"):
        raise RuntimeError("libmi355x_probe.so predates the host-link check: rebuild it")
    opts = {"hostLinkBytes": int(nbytes), "hostLinkPatterns": int(patterns),
            **{k: int(v) for k, v in hooks.items()}}
    buf, n = None, 0
    if preload is not None:
        raw = bytes(preload) if not hasattr(preload, "tobytes") else preload.tobytes()
        n = len(raw)
        buf = ctypes.create_string_buffer(raw, n)
        opts["preload"] = 1
    elif want_bytes > 0:
        n = int(want_bytes)
        buf = ctypes.create_string_buffer(n)
    res = _take(lib().mi355x_probe_host_link(dev, json.dumps(opts).encode(), buf, n))
    if buf is not None and want_bytes > 0 and "bytes" in res:
        res["data"] = buf.raw[:min(int(want_bytes), n, int(res["bytes"]))]
    return res


def lds(dev: int, nbytes: int = 163840, patterns: int = 2, want_stage: int = 0, **hooks: int) -> dict:
    """The LDS phase alone (``mi355x_probe_lds``): every CU's Local Data Share marched over its
    first ``nbytes`` (16 .. 163840, rounded down to 16) in ``patterns`` polarities and
    address-tested. -> the "lds" block of ``run`` plus "device" and "passed". ``want_stage`` 1 | 2
    | 3: workgroup 0's LDS as it stood after the first write / after the first complement write /
    after the address pass's stores comes back under "data" (bytes; ``gpupool.ops.lds`` is its
    numpy twin) and "dumpCU" names the CU it ran on. ``hooks``: ldsSalt, ldsBlocksPerCU,
    requireAllCUs, injectLdsFlipAtByte, injectLdsFaultXcc, injectLdsSkipChunk."""
    if not hasattr(lib(), "mi355x_probe_lds"):
        raise RuntimeError("libmi355x_probe.so predates the LDS check: rebuild it")
    opts = {"ldsBytes": int(nbytes), "ldsPatterns": int(patterns), **{k: int(v) for k, v in hooks.items()}}
    buf, n = None, 0
    if want_stage:
        opts["ldsDumpStage"] = int(want_stage)
        n = 163840
        buf = ctypes.create_string_buffer(n)
    res = _take(lib().mi355x_probe_lds(dev, json.dumps(opts).encode(), buf, n))
    if buf is not None and "bytesPerCU" in res:
        res["data"] = buf.raw[:int(res["bytesPerCU"])]
    return res


def regs(dev: int, patterns: int = 2, want_stage: int = 0, **hooks) -> dict:
    """The register-file phase alone (``mi355x_probe_regs``): the 512 vector registers (v0..v255,
    a0..a255) of every lane of every SIMD of every CU marched in ``patterns`` polarities. -> the
    "regs" block of ``run`` plus "device" and "passed". ``want_stage`` 1 | 2: workgroup 0's
    registers as they stood after the first write / after the first complement write come back
    under "data" (uint32 [4][512][64]: wave, register, lane; ``gpupool.ops.regfile`` is the numpy
    twin), "dumpCU" names the CU it ran on and "dumpSimds" the SIMD of each of its waves.
    ``hooks``: regsSalt, regsBlocksPerCU, requireAllCUs, injectRegFlip=[u, lane, bit],
    injectRegFaultSimd, injectRegFaultXcc, injectRegSkip."""
    import numpy as np

    from . import regfile
    if not hasattr(lib(), "mi355x_probe_regs"):
        raise RuntimeError("libmi355x_probe.so predates the register-file check: rebuild it")
    opts = {"regsPatterns": int(patterns), **{k: _hook(v) for k, v in hooks.items()}}
    buf, n = None, 0
    if want_stage:
        opts["regsDumpStage"] = int(want_stage)
        n = regfile.IMAGE_BYTES
        buf = ctypes.create_string_buffer(n)
    res = _take(lib().mi355x_probe_regs(dev, json.dumps(opts).encode(), buf, n))
    if buf is not None and "dumpCU" in res:
        res["data"] = np.frombuffer(buf.raw, dtype="<u4").reshape(regfile.WAVES, regfile.REGISTERS,
                                                                   regfile.LANES).copy()
    return res


def alu(dev: int, iters: int | None = None, want_stage: int = 0, **hooks) -> dict:
    """The vector-ALU phase alone (``mi355x_probe_alu``): the instruction program of
    native/src/probe/alu.h on every SIMD of every CU, ``iters`` steps per group (default: the
    library's). -> the "alu" block of ``run`` plus "device" and "passed". ``want_stage`` 1 | 2:
    workgroup 0's digests after step 0 / after the last step come back under "data" (uint32
    [4][6][64]: wave, group, lane; ``gpupool.ops.alu`` is the exact twin of the first five groups),
    "dumpCU" names the CU it ran on and "dumpSimds" the SIMD of each of its waves. ``want_stage`` 3:
    "data" is workgroup 0's trace of the trans group instead, uint32 [4][64][12][64] (wave, step, word,
    lane) of the first min(iters, 64) steps and zero past them: word 0 the lane's digest as the step
    began, words 1..11 the step's results as they were folded (``gpupool.ops.alu.TRANS_WORDS``; the
    probe itself judges trans by consensus only, the tests compare this trace with
    ``gpupool.ops.alu.trans_reference``). ``hooks``:
    aluBlocksPerCU, aluSeed, requireAllCUs, injectAluFlip=[group, step, lane, bit],
    injectAluFaultSimd, injectAluFaultXcc."""
    import numpy as np

    from . import alu as twin
    if not hasattr(lib(), "mi355x_probe_alu"):
        raise RuntimeError("libmi355x_probe.so predates the vector-ALU check: rebuild it")
    opts = {**({"aluIters": int(iters)} if iters is not None else {}), **{k: _hook(v) for k, v in hooks.items()}}
    buf, n = None, 0
    shape = (twin.WAVES, len(twin.GROUPS), twin.LANES)
    if want_stage:
        opts["aluDumpStage"] = int(want_stage)
        n = twin.DUMP_BYTES
        if int(want_stage) == 3:
            n, shape = twin.TRACE_BYTES, (twin.WAVES, twin.TRACE_STEPS, twin.TRACE_WORDS, twin.LANES)
        buf = ctypes.create_string_buffer(n)
    res = _take(lib().mi355x_probe_alu(dev, json.dumps(opts).encode(), buf, n))
    if buf is not None and "dumpCU" in res:
        res["data"] = np.frombuffer(buf.raw, dtype="<u4").reshape(shape).copy()
    return res


def atomics(dev: int, iters: int | None = None, want_stage: int = 0, **hooks) -> dict:
    """The atomic-unit phase alone (``mi355x_probe_atomics``): the program of
    native/src/probe/atomics.h on every CU, ``iters`` steps per layer (default: the library's). -> the
    "atomics" block of ``run`` plus "device" and "passed". ``want_stage`` 1 | 2: workgroup 0's data comes
    back as uint32 arrays: "ldsTable" [2688], "ldsTable16" [1408] (the second addressing), "ldsDigests"
    and "l2Digests" [4][64] as they stood after step 0 / after the last step, and, of the whole run either
    way, "region" [2688] and "devRows" [9][1408] as the verifying kernel read them, and
    "wgKeys" / "wgXcc", the CU key and the XCD of each workgroup's record (``gpupool.ops.atomics`` is the
    twin of all of them); "dumpCU"
    names the CU it ran on and "dumpSimds" the SIMD of each of its waves. ``hooks``: atomBlocksPerCU,
    atomLayers, atomSeed, requireAllCUs, atomTimeKernels (adds "marchMs" and "verifyMs", each kernel's time),
    injectAtomSkip=[layer, op, step, lane], injectAtomFlip=[layer,
    op, step, lane, bit], injectAtomFaultXcc, injectAtomFaultWorkgroup."""
    import numpy as np

    from . import atomics as twin
    if not hasattr(lib(), "mi355x_probe_atomics"):
        raise RuntimeError("libmi355x_probe.so predates the atomic-unit check: rebuild it")
    opts = {**({"atomIters": int(iters)} if iters is not None else {}), **{k: _hook(v) for k, v in hooks.items()}}
    buf, n = None, 0
    if want_stage:
        opts["atomDumpStage"] = int(want_stage)
        n = twin.DUMP_BYTES
        buf = ctypes.create_string_buffer(n)
    res = _take(lib().mi355x_probe_atomics(dev, json.dumps(opts).encode(), buf, n))
    if buf is not None and "dumpCU" in res:
        w = np.frombuffer(buf.raw, dtype="<u4").copy()
        res["ldsTable"] = w[twin.DUMP_LDS:twin.DUMP_LDS_DIGEST]
        res["ldsTable16"] = w[twin.DUMP_LDS16:twin.DUMP_WORDS]
        res["ldsDigests"] = w[twin.DUMP_LDS_DIGEST:twin.DUMP_L2_DIGEST].reshape(twin.WAVES, twin.LANES)
        res["l2Digests"] = w[twin.DUMP_L2_DIGEST:twin.DUMP_REGION].reshape(twin.WAVES, twin.LANES)
        res["region"] = w[twin.DUMP_REGION:twin.DUMP_DEV]
        res["devRows"] = w[twin.DUMP_DEV:twin.DUMP_RECORDS].reshape(twin.DEV_ROWSETS, twin.ROWSET_WORDS)
        res["wgKeys"] = w[twin.DUMP_RECORDS:twin.DUMP_RECORDS + int(res["workgroups"])].tolist()
        res["wgXcc"] = [k >> 8 for k in res["wgKeys"]]
    return res


def peer(src: int, dst: int, nbytes: int = 64 << 20, want_bytes: int = 0, **hooks: int) -> dict:
    """xGMI peer check src -> dst: pattern written on src, hipMemcpyPeer over the link, every bit
    verified on dst; reports GB/s, "firstBadOffset" and the per-call "seed" it verified with.
    ``src == dst`` exercises the same path as a local copy. ``want_bytes`` > 0: the first
    ``min(want_bytes, tested bytes)`` of the destination buffer after the verify come back under
    "data" (bytes; ``gpupool.ops.hostlink.pattern_bytes`` with the reported seed is their numpy
    twin). ``hooks`` (test hooks): injectFlipAtChunk=i / injectBitFlips=k corrupt the destination
    between the copy and the verify, skipCopy=1 leaves the copy out."""
    opts = json.dumps({"bytes": int(nbytes), **{k: int(v) for k, v in hooks.items()}}).encode()
    if want_bytes <= 0:
        return _take(lib().mi355x_probe_peer(src, dst, opts))
    if not hasattr(lib(), "mi355x_probe_peer_dump"):
        raise RuntimeError("libmi355x_probe.so predates the peer check's dump: rebuild it")
    n = int(want_bytes)
    buf = ctypes.create_string_buffer(n)
    res = _take(lib().mi355x_probe_peer_dump(src, dst, opts, buf, n))
    if "bytes" in res:
        res["data"] = buf.raw[:min(n, int(res["bytes"]))]
    return res


def peer_ring(ordinals: list[int], nbytes: int = 64 << 20, **hooks: int) -> dict:
    """The xGMI ring in one call: link i copies ordinals[i] -> ordinals[i+1] (wrapping), every link
    concurrently, then each receiver verifies every bit. -> {"links": [...], "passed"}. ``hooks``
    (test hooks): injectFlipAtChunk=i / injectBitFlips=k corrupt the receive window of link
    injectLink=j (default 0) ahead of its verify, skipCopy=1 leaves every link's copy out."""
    n = len(ordinals)
    if n < 2:
        raise ValueError("a ring needs at least 2 entries")
    if not hasattr(lib(), "mi355x_probe_peer_ring"):
        raise RuntimeError("libmi355x_probe.so predates the ring check: rebuild it")
    arr = (ctypes.c_int * n)(*[int(o) for o in ordinals])
    opts = json.dumps({"bytes": int(nbytes), **{k: int(v) for k, v in hooks.items()}})
    return _take(lib().mi355x_probe_peer_ring(arr, n, opts.encode()))


def hip_uuid_map() -> dict[str, int]:
    """hipUUID ("GPU-<serial>") -> HIP ordinal for every visible device."""
    n = init()
    out = {}
    for d in range(n):
        info = identify(d)
        if info.get("hipUUID"):
            out[info["hipUUID"].lower()] = d
    return out


def trim(idle_ms: int = 0) -> int:
    """Free the probe arenas (kept between probes to skip a ~1.2 GiB hipMalloc) that have been idle
    for at least ``idle_ms``; returns how many were freed."""
    return int(lib().mi355x_probe_trim(int(idle_ms)))


def hbm_sweep(dev: int, offset: int, nbytes: int = 16 << 30, reserve: int = 4 << 30,
              keep: bool = False, **test_hooks: int) -> dict:
    """Pattern-test HBM window [offset, offset+nbytes) of a buffer spanning all free HBM minus
    ``reserve`` (the rotating sweep that covers the whole 288 GB over successive calls). With
    ``keep`` the big buffer stays allocated for the next window (free it with sweep_release).
    ``test_hooks``: injectBitFlips=k (spread over the window's first piece), injectFlipAtChunk=i
    (bit 0 of 16-byte chunk i counted from the window's start, in whichever 1 GiB chunk of the
    buffer holds it; past the window: no flip)."""
    opts = json.dumps({"offset": int(offset), "bytes": int(nbytes), "reserve": int(reserve),
                       "keep": bool(keep), **{k: int(v) for k, v in test_hooks.items()}})
    return _take(lib().mi355x_probe_hbm_sweep(dev, opts.encode()))


def sweep_alloc(dev: int, reserve: int = 4 << 30) -> int:
    """Allocate the sweep buffer (all free HBM minus ``reserve``) without blocking probes: 1
    allocated, 0 already held, < 0 error."""
    return int(lib().mi355x_probe_sweep_alloc(dev, int(reserve)))


def sweep_release(dev: int) -> int:
    """Free the sweep buffer (seconds for ~280 GB; probes of the device are not blocked)."""
    return int(lib().mi355x_probe_sweep_release(dev))


_GEMM_OPTS = {"gemm_tile": "gemmTile", "gemm_pipe": "gemmPipe", "gemm_prio": "gemmPrio",
              "gemm_vec_c": "gemmVecC", "gemm_group_m": "gemmGroupM", "poison_c": "poisonC"}


def gemm_bf16(dev: int, a_ptr: int, bt_ptr: int, c_ptr: int, m: int, n: int, k: int,
              **opts: int) -> None:
    """One of the probe's MFMA GEMM kernels on caller HOST buffers (C fp32 [m,n] = A bf16 [m,k] x
    Bt bf16 [n,k]^T; e.g. CPU torch tensors' ``data_ptr()``), for independent numerics checks.
    Without options: the production kernel, as the claim-time probe launches it. Options (meanings
    and defaults as for ``run``): ``gemm_tile`` 256 | 128, ``gemm_pipe`` 0 | 1 | 2 | 3 | 21 | 22,
    ``gemm_prio``, ``gemm_vec_c``, ``gemm_group_m``, and ``poison_c`` (the device C starts as 0xFF
    bytes, so an unwritten tile comes back as NaN). Tile 256 needs m, n % 256 == 0 and k % 64 == 0,
    tile 128 m, n % 128 == 0 and k % 32 == 0; a timing-only pipe (11, 12) is refused."""
    unknown = sorted(set(opts) - set(_GEMM_OPTS))
    if unknown:
        raise TypeError(f"gemm_bf16: unknown option(s) {unknown}")
    if not opts:
        rc = lib().mi355x_probe_gemm_bf16(dev, a_ptr, bt_ptr, c_ptr, m, n, k)
    else:
        if not hasattr(lib(), "mi355x_probe_gemm_bf16_opts"):
            raise RuntimeError("libmi355x_probe.so predates the GEMM options: rebuild it")
        js = json.dumps({_GEMM_OPTS[key]: int(v) for key, v in opts.items()}).encode()
        rc = lib().mi355x_probe_gemm_bf16_opts(dev, a_ptr, bt_ptr, c_ptr, m, n, k, js)
    if rc == -4:
        raise RuntimeError("mi355x_probe_gemm_bf16 failed with a HIP error (rc=-4)")
    if rc != 0:
        raise ValueError(f"mi355x_probe_gemm_bf16 refused its arguments (rc={rc}): m, n must be "
                         f"multiples of the tile (256 | 128), k of 64 | 32, the pipe one that "
                         f"computes C and the device index valid")


def gemm_lowp(dev: int, dtype: str, a_ptr: int, bt_ptr: int, scale_a_ptr: int | None,
              scale_bt_ptr: int | None, c_ptr: int, m: int, n: int, k: int, poison_c: int = 0) -> None:
    """The probe's low-precision MFMA GEMM on caller HOST buffers: C fp32 [m,n] = A [m,k] x Bt [n,k]^T
    with ``dtype`` "fp8" | "mxfp8" (one e4m3 byte per element) | "mxfp4" (two e2m1 per byte, rows of
    k/2 bytes); ``scale_*_ptr``: [rows][k/32] E8M0 bytes, None for "fp8". m, n, k multiples of 128.
    Layouts and codecs: ``gpupool.ops.lowp``. A refused call (ValueError) leaves C untouched."""
    if not hasattr(lib(), "mi355x_probe_gemm_lowp"):
        raise RuntimeError("libmi355x_probe.so predates the low-precision GEMM: rebuild it")
    js = json.dumps({"poisonC": int(poison_c)}).encode()
    rc = lib().mi355x_probe_gemm_lowp(dev, lowp.dtype_index(dtype), a_ptr, bt_ptr, scale_a_ptr,
                                      scale_bt_ptr, c_ptr, m, n, k, js)
    if rc == -4:
        raise RuntimeError("mi355x_probe_gemm_lowp failed with a HIP error (rc=-4)")
    if rc != 0:
        raise ValueError(f"mi355x_probe_gemm_lowp refused its arguments (rc={rc}): m, n, k must be "
                         f"multiples of 128, scales given exactly for the scaled dtypes and the "
                         f"device index valid")


# ---------------------------------------------------------------- test surfaces of the checkers
# The kernels that decide a probe's verdict, on caller HOST buffers (pointers as for gemm_lowp), so a
# test can compare them with a host reference (tests/gpu/abft_cases.py). Not on the claim path.
def _checker_dtype(dtype: str) -> int:
    return -1 if dtype == "bf16" else lowp.dtype_index(dtype)


def _checker_rc(name: str, rc: int) -> None:
    if rc == -4:
        raise RuntimeError(f"mi355x_probe_{name} failed with a HIP error (rc=-4)")
    if rc != 0:
        raise ValueError(f"mi355x_probe_{name} refused its arguments (rc={rc})")


def _checker_lib():
    if not hasattr(lib(), "mi355x_probe_abft_check"):
        raise RuntimeError("libmi355x_probe.so predates the checker test surfaces: rebuild it")
    return lib()


def abft_check(dev: int, dtype: str, a_ptr: int, bt_ptr: int, scale_a_ptr: int | None,
               scale_bt_ptr: int | None, c_ptr: int, m: int, n: int, k: int, bound: float,
               vectors_ptr: int, counts_ptr: int, nfaults: int = 0, fault_index_ptr: int | None = None,
               fault_value_ptr: int | None = None, fault_counts_ptr: int | None = None) -> None:
    """The probe's ABFT checker sequence over A [m,k], Bt [n,k] (``dtype`` "bf16" or one of
    ``lowp.DTYPES``) and the caller's C fp32 [m,n]. ``vectors_ptr``: 2k + 2n + 2m uint32 (column sums
    of A, of Bt, of C, expected of C; row sums of C, expected), ``counts_ptr``: 3 uint64 (elements
    that are no integer / not finite / beyond ``bound``, column mismatches, row mismatches).
    ``nfaults`` > 0: per fault i, C[fault_index[i]] (int64, row * n + col) is set to fault_value[i]
    (float32) on the device, the sequence runs, the element is put back; ``fault_counts_ptr``:
    3 * nfaults uint64. bf16 k % 8 == 0, else k % 32 == 0; n % 4 == 0. A refused call (ValueError)
    leaves every output untouched."""
    _checker_rc("abft_check", _checker_lib().mi355x_probe_abft_check(
        dev, _checker_dtype(dtype), a_ptr, bt_ptr, scale_a_ptr, scale_bt_ptr, c_ptr, m, n, k, bound,
        vectors_ptr, counts_ptr, nfaults, fault_index_ptr, fault_value_ptr, fault_counts_ptr))


def gemm_ref(dev: int, dtype: str, a_ptr: int, bt_ptr: int, scale_a_ptr: int | None,
             scale_bt_ptr: int | None, r_ptr: int, m: int, n: int, k: int) -> None:
    """The VALU reference of the probe's element check: R fp32 [m,n] = A x Bt^T, shapes and dtypes
    as for ``abft_check``."""
    _checker_rc("gemm_ref", _checker_lib().mi355x_probe_gemm_ref(
        dev, _checker_dtype(dtype), a_ptr, bt_ptr, scale_a_ptr, scale_bt_ptr, r_ptr, m, n, k))


def count_diff(dev: int, x_ptr: int, y_ptr: int, count: int) -> int:
    """How many of ``count`` float32 elements the element check's comparer finds different."""
    bad = ctypes.c_ulonglong(0)
    _checker_rc("count_diff", _checker_lib().mi355x_probe_count_diff(dev, x_ptr, y_ptr, count,
                                                                     ctypes.byref(bad)))
    return int(bad.value)


def gen_operands(dev: int, dtype: str, seed: int, span_or_scale_lo: int, count: int, nzero: int,
                 operand_ptr: int, operand_bytes: int, scales_ptr: int | None = None,
                 scale_bytes: int = 0, zero_ptr: int | None = None, zero_bytes: int = 0) -> None:
    """The in-probe operand generator with its production grid, into device buffers that start as
    0xFF bytes and come back whole: ``count`` elements ("bf16": integers in [-span, span]; low
    precision: whole 32-bit words, count / 32 scale bytes for the scaled dtypes) and, bf16 only,
    the first ``nzero`` words of the zero region zeroed."""
    _checker_rc("gen_operands", _checker_lib().mi355x_probe_gen_operands(
        dev, _checker_dtype(dtype), seed, span_or_scale_lo, count, nzero, operand_ptr, operand_bytes,
        scales_ptr, scale_bytes, zero_ptr, zero_bytes))
