/* libmi355x_probe — HIP readiness probe for MI355X (gfx950). See native/src/probe/probe.hip.
 *
 * The node agent loads this once (ctypes) and calls mi355x_probe_init() at start-up so every
 * device context is warm; a claim-time probe then costs only its kernels (HBM pattern
 * fill/verify + bf16 MFMA GEMM checks), not HIP runtime initialisation.
 * Device indices are HIP ordinals within the calling process's visible set.
 */
#ifndef MI355X_PROBE_H_
#define MI355X_PROBE_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Returns the number of HIP devices (>= 0) or -1 with a message in err. Idempotent. */
int mi355x_probe_init(char* err, size_t errlen);
int mi355x_probe_device_count(void);
/* {"device","hipUUID","name","gcnArch","bdf","totalMem","computeUnits"} */
char* mi355x_probe_identify(int device);
/* opts: {"hbmBytes":1073741824,"patterns":2,"mfma":true,"gemmN":4096,"gemmReps":3,
 *        "requireAllCUs":true}
 * -> {"passed":bool,"hbm":{...,"GBps"},"mfma":{...,"tflops"},
 *     "cus":{"expected","mfmaVerified","perXcd":[8],"gemmTiles","badWaves","ok"},"ms":...}
 * cus: every CU's matrix cores are exercised by a census kernel (chained MFMAs checked exactly per
 * wave, the CU identified by its XCC_ID/HW_ID registers); with requireAllCUs the probe fails
 * unless mfmaVerified >= the runtime's CU count. gemmTiles = CUs that ran tiles of the timed GEMM.
 * Test hooks (corrupt a buffer between compute and check): "injectBitFlips":N flips N bits spread
 * over the HBM region, "injectFlipAtChunk":i flips bit 0 of 16-byte chunk i, "injectGemmFault":mode
 * (1: +1.0, 2: +0.25, else NaN) at one element of the gemmN GEMM's C: "injectGemmFaultRow" /
 * "injectGemmFaultCol", -1 (default) row gemmN/3 and column gemmN/5, any other value outside
 * [0, gemmN) no fault. "injectLowpFault" strikes the same element.
 *
 * Low-precision matrix cores (opt-in): "mfmaLowPrecision":mask, bit 0 fp8 (OCP e4m3fn on
 * v_mfma_f32_16x16x32_fp8_fp8), bit 1 mxfp8 (e4m3) and bit 2 mxfp4 (e2m1), both on
 * v_mfma_scale_f32_16x16x128_f8f6f4 with an E8M0 scale per 32 K-elements. Ignored with "mfma":false.
 * Each dtype adds, after the bf16 phase on its stream: a per-CU census on that instruction, a 256^3
 * GEMM checked element by element against a VALU reference, and the gemmN GEMM with exact ABFT. The
 * report then gains
 *   "lowp":{"<dtype>":{"ok","n","elementMismatches","abftMismatches","tflops","ms","cusVerified",
 *                      "badWaves"}}
 * and "passed" also needs every entry's "ok". Without the option: no "lowp" key, no extra launch,
 * the same arena. Test hooks: "injectLowpFault":mask (+1.0 at one element of those dtypes' C),
 * "injectLowpCensusFaultXcc":x.
 *
 * Host link (opt-in): "hostLinkBytes":N (0 / absent: off) tests N / 16 chunks of a pinned, device-mapped
 * host buffer over PCIe: per pass the GPU writes the HBM test's address-dependent pattern into host
 * memory (device -> host), reads it back (host -> device) and verifies every bit; "hostLinkPatterns"
 * passes (default 2, 1..4), odd passes in the complementary polarity, seed 0x4C4B0000 + device. After
 * the final synchronise the host recomputes the last pass's pattern at 1024 evenly spaced chunks plus
 * the first and the last and compares them with its DRAM. With "overlap" the phase runs on a stream of
 * its own beside the HBM and MFMA phases; with "overlap":0 last on the one stream, alone on the GPU.
 * The report then gains
 *   "hostLink":{"ok","bytes","patterns","seed","badBits","firstBadOffset","hostSamples",
 *               "hostSampleMismatches","writeGBps","readGBps","GBps","ms","allocMs"}
 * writeGBps device -> host, readGBps host -> device, GBps the slower of the two; allocMs the pinned
 * allocation's cost when this probe made or grew it, else 0; ok = no bad bit and no sample mismatch,
 * and "passed" also needs it. The buffer, the stream and the events are made by the first probe that
 * asks, the buffer grown when a larger size is asked for, never shrunk and never trimmed. Without the
 * option: no "hostLink" key, no extra launch, allocation, stream or event. Test hook:
 * "injectHostLinkFlipAtChunk":i — once the first write pass has completed (the one case with a
 * stream synchronise inside the phase) the HOST flips bit 0 of chunk i; out of range: no flip.
 * A/B knobs of the measurement sweep: "hostLinkGrid", "hostLinkUnroll" (4 | 8 | 16), "hostLinkNT",
 * "hostLinkCoherent", "hostLinkStream" (1: the tail of the MFMA stream).
 *
 * LDS (opt-in): "ldsCheck":1 tests the Local Data Share of every CU. One kernel of 256-thread workgroups,
 * each declaring the CU's whole 163,840-byte LDS (so it has the CU's LDS to itself), "ldsBlocksPerCU" of
 * them per CU: per polarity ("ldsPatterns", default 2, 1..4) a march — write the workgroup- and
 * address-dependent pattern, verify it from another wave and write the complement, verify that from a
 * third — then an address pass at dword granularity through 4-byte stores in a strided order, read back
 * 16 bytes at a time. "ldsBytes" (default and maximum 163840, at least 16, rounded down to 16) is what of
 * the LDS is tested; seed (0x4C445300 + device) ^ "ldsSalt" (default: a per-device run counter). It runs on
 * the MFMA stream ahead of the MFMA phase ("ldsFirst":0 behind it and the low-precision phases), with
 * "overlap":0 last on the one stream. The report then gains, after "hostLink",
 *   "lds":{"ok","bytesPerCU","patterns","salt","workgroups","cusTested","cusVerified","perXcd","badCUs",
 *          "badBits","firstBadCU","firstBadOffset","ms"}
 * cusVerified = tested and not bad, perXcd the verified CUs per XCD, firstBadCU the 11-bit CU key
 * (xcc[10:8] se[7:5] sh[4] cu[3:0]) and firstBadOffset the byte offset of the lowest fault or null;
 * ok = no bad bit and, unless "requireAllCUs":0, every CU verified; "passed" also needs it. Without the
 * option: no "lds" key, no launch, allocation or event. Test hooks, all plain LDS stores:
 * "injectLdsFlipAtByte":o (bit 0 of byte o in every workgroup after the first write; out of range: none),
 * "injectLdsFaultXcc":x (that flip only on XCD x), "injectLdsSkipChunk":j (the first write leaves chunk j).
 *
 * Register files (opt-in): "regCheck":1 tests the vector register file of every SIMD of every CU: the 512
 * registers per lane (v0..v255 numbered u = 0..255, a0..a255 numbered 256..511) of all 64 lanes. One kernel
 * of 256-thread workgroups whose descriptor asks for all 512 registers, so a SIMD holds one wave of it and a
 * workgroup has its CU to itself, "regsBlocksPerCU" of them per CU (default 2, 1..64). Register u of lane l of
 * wave w of workgroup b is expected to hold (base + u * 0x9E3779B1) ^ flip, base the first word of pattern16
 * of index (b << 32) | (64 w + l), seed (0x52454700 + device) ^ "regsSalt" (default: a per-device run
 * counter). Per polarity ("regsPatterns", default 2, 1..4): write every register ascending, verify each
 * ascending and write its complement (computed from the expected value), verify the complements descending.
 * AGPRs are moved only by v_accvgpr_write_b32 / v_accvgpr_read_b32; the march is two asm statements, one over
 * v16..v255 and a0..a255 with the compiler's operands below v16, one over v0..v15. It runs on the MFMA stream
 * behind the MFMA and low-precision phases ("regsFirst":1 ahead of them), behind the LDS phase where both
 * are asked for, with "overlap":0 last on the one stream. The report then gains, after "lds",
 *   "regs":{"ok","registersPerLane","workgroupsPerCU","patterns","salt","workgroups","cusTested","cusVerified",
 *           "simdsTested","simdShort","perXcd","badCUs","badBits","firstBadCU","firstBadSimd",
 *           "firstBadRegister","firstBadLane","ms"}
 * registersPerLane / workgroupsPerCU are what the runtime says of the kernel (hipFuncGetAttributes,
 * hipOccupancyMaxActiveBlocksPerMultiprocessor): anything but 512 and 1 fails the phase and adds
 * "error":"RegisterKernelNotExclusive" to the block. A workgroup marks its CU tested only when its four
 * waves read four different SIMD ids (HW_ID[5:4]), else it counts into simdShort; simdsTested = 4 x
 * cusTested; cusVerified = tested and not bad, perXcd the verified CUs per XCD; firstBadCU (the 11-bit CU
 * key), firstBadSimd, firstBadRegister (the unified index u) and firstBadLane name the lowest fault, or are
 * null. ok = no bad bit, the kernel exclusive, simdShort 0 and, unless "requireAllCUs":0, every CU verified;
 * "passed" also needs it. Without the option: no "regs" key, no launch, allocation or event. Test hooks (any
 * of them, or the dump below, selects the kernel's test instantiation; the production one carries none):
 * "injectRegFlip":[u, lane, bit] (that bit of register u in that lane of every wave, after the first write),
 * "injectRegFaultSimd":s / "injectRegFaultXcc":x (that flip only on SIMD s / on XCD x), "injectRegSkip":u
 * (the first write leaves register u alone); a value out of range switches its hook off. */
char* mi355x_probe_run(int device, const char* opts_json);
/* The register-file phase alone, on the device's first stream, under the device's probe lock; the "regs"
 * block (after "device" and "passed") is the whole report. opts as above (without "regCheck"). With image
 * and "regsDumpStage":1|2, workgroup 0's registers are stored to a device image uint32[4][512][64] (wave,
 * register u, lane) — 1 after the first write, 2 after the first complement write — whose first
 * min(image_bytes, 524288) bytes land in image, and the report names "dumpCU", the CU key that workgroup ran
 * on, and "dumpSimds", the SIMD of each of its four waves. A bad device: {"passed":false,"error":...}. */
char* mi355x_probe_regs(int device, const char* opts_json, void* image, size_t image_bytes);
/* Vector ALUs (opt-in): "aluCheck":1 in mi355x_probe_run's options runs a fixed program of vector-ALU
 * instructions on every SIMD of every CU: one kernel of 256-thread workgroups with ordinary register counts,
 * "aluBlocksPerCU" of them per CU (1..64). Six groups (0 int, 1 f32, 2 f64, 3 f16, 4 lane, 5 trans) of
 * "aluIters" steps (1..4096) over a 32-bit digest per lane and group; every operand of a step is
 * pattern_word(group << 32 | step << 12 | operand << 6 | lane, seed) ^ digest, every result is folded into the
 * digest, (rotl(h, 5) ^ r) * 0x9E3779B1. The seed is 0x414C5500 + device ("aluSeed" overrides it) and is not
 * salted per run: the library computes the expected digests of the five exact groups on the host
 * (native/src/probe/alu_ref.h) once per context and (seed, iters) and every lane compares its own with
 * them. The transcendental group is compared with the device-wide consensus: the first wave publishes its
 * 64-bit digest, every other wave compares. The phase rides the MFMA stream behind the MFMA and
 * low-precision phases ("aluFirst":1 ahead of them), behind the LDS and register-file phases where asked
 * for, with "overlap":0 last on the one stream. The report then gains, after "regs",
 *   "alu":{"ok","iters","workgroups","waves","wavesPerSimd","simdsTested","simdsVerified","cusVerified","perXcd",
 *          "badWaves","badLanes","badCUs","firstBadCU","firstBadSimd","firstBadGroup","firstBadLane","splitWaves",
 *          "suspectCU","suspectSimd","transDigest","ms"}
 * wavesPerSimd: the waves that ran on SIMD 0..3 of their CU (HW_ID[5:4]), waves their sum; a wave whose every
 * check passed marks its (CU, SIMD) verified, one that failed marks it bad: simdsTested = either,
 * simdsVerified = verified and not bad, perXcd those per XCD, cusVerified the CUs with all four. badWaves /
 * badLanes count mismatches against the host, badCUs the CUs with a SIMD marked bad; firstBadCU (the 11-bit CU key), firstBadSimd, firstBadGroup (a
 * name) and firstBadLane name the lowest, or are null. splitWaves counts the waves whose transcendental
 * digest differs from the published one, transDigest (16 hex digits); suspectCU / suspectSimd name the
 * publisher when more than half of the waves differ and the first differing wave otherwise (null without a
 * split). ok = badWaves 0, splitWaves 0 and, unless "requireAllCUs":0, simdsVerified = 4 x CUs; "passed" also
 * needs it. Without the option: no "alu" key, no launch, allocation or event. Test hooks (either, or the dump
 * below, selects the kernel's test instantiation): "injectAluFlip":[group, step, lane, bit] XORs that bit into
 * the last result of that step of that group in that lane of every wave, "injectAluFaultSimd":s /
 * "injectAluFaultXcc":x only on SIMD s / on XCD x; a value out of range switches the hook off.
 *
 * mi355x_probe_alu: the phase alone, on the device's first stream, under the device's probe lock; the "alu"
 * block (after "device" and "passed") is the whole report. opts as above (without "aluCheck"). With dump and
 * "aluDumpStage":1|2, workgroup 0's digests uint32[4][6][64] (wave, group, lane) after step 0 / after the
 * last step land in dump (the first min(dump_bytes, 6144) bytes), and the report names "dumpCU" and
 * "dumpSimds" as mi355x_probe_regs does. "aluDumpStage":3 returns workgroup 0's raw-result trace of the
 * transcendental group instead, uint32[4][64][12][64] (wave, step, word, lane; the first min(dump_bytes, 786432)
 * bytes), from a device buffer of its own that is zeroed ahead of the launch: the first min(iters, 64) steps, word 0
 * the lane's trans digest as the step began, words 1..11 the step's results exactly as they were folded (the
 * "injectAluFlip" XOR included): exp2(a), log2|b|, rcp(a), rsq|b|, sqrt|a|, sin(a), cos(b), rcp(q) low, high,
 * rsq|q| low, high; "dumpCU" and "dumpSimds" as for the other stages. The probe's verdict on that group stays the
 * consensus; the trace is what the test suite compares with a reference of the nine functions. A bad device:
 * {"passed":false,"error":...}. */
char* mi355x_probe_alu(int device, const char* opts_json, void* dump, size_t dump_bytes);
/* Atomic units (opt-in): "atomCheck":1 in mi355x_probe_run's options runs a fixed program of read-modify-write
 * instructions on every CU: atom_march, 256-thread workgroups with ordinary register counts, "atomBlocksPerCU" of
 * them per CU (1..16), "atomIters" steps (1..64) per layer, then atom_verify on the same stream. "atomLayers" is
 * a mask (default 7): 1 lds — the CU's LDS atomic unit, a table in LDS the four waves contend on, returning ops
 * on words private to a lane with a digest of everything returned, a second addressing slot = lane & 15 that
 * puts four lanes of every wave on one word (a fault there is slot 64 + (lane & 15)), and a ticket test under
 * full contention; 2 l2
 * — the same program through global atomics at agent scope on a region private to the workgroup; 4 dev — the
 * contended ops on nine row-sets, one every workgroup hits and one per XCD. Ops (a fault's "firstBadOp"): 0 add,
 * 1 sub, 2 and, 3 or, 4 xor, 5 umin, 6 umax, 7 smin, 8 smax, 9 add_f32, 10 pk_add_f16, 11 pk_add_bf16, 12 add_x2,
 * 13 umax_x2, 14 xor_x2, 15 add_f64, 16 max_f64 (contended, slot = lane), 17 add_rtn, 18 inc, 19 dec, 20 swap,
 * 21 cas (returning, not in the dev layer), 22 ticket, 23 returns (a lane's digest; slot = wave * 64 + lane).
 * Every operand is derived from pattern_word(layer << 40 | op << 32 | step << 10 | part << 8 | wave << 6 | lane,
 * seed) as native/src/probe/atomics_ref.h documents; floating-point operands are small integers, so every
 * partial sum in every arrival order is exact. The seed is 0x41544D00 + device ("atomSeed" overrides it) and is
 * not salted per run: the library computes the expectation on the host once per context and (seed, iters).
 * atom_verify compares every final value and stores every word's initial value back. The phase rides the MFMA
 * stream behind every other phase there ("atomFirst":1 ahead of the MFMA phase), with "overlap":0 last on the
 * one stream. The report then gains, after "alu",
 *   "atomics":{"ok","iters","layers","workgroups","wgPerXcd","cusTested","cusVerified","perXcd","badCUs",
 *              "badWorkgroups","ldsBadSlots","l2BadSlots","devBadSlots","badReturns","ticketFaults","firstBadCU",
 *              "firstBadLayer","firstBadOp","firstBadSlot","firstBadXcc","ms"}
 * wgPerXcd: the workgroups that ran on XCD 0..7, workgroups their sum. cusTested: CUs a workgroup ran on;
 * badCUs: CUs a workgroup with an lds or l2 mismatch, a bad digest or a ticket fault ran on; cusVerified = tested
 * and not bad, perXcd those per XCD. *BadSlots count slots (4 or 8 bytes) off the expectation, badReturns lanes
 * whose digest is, ticketFaults workgroups whose ticket word is not 256 or whose map is not all ones.
 * firstBad* name the lowest (layer, op, slot, row) or are null; firstBadCU is the 11-bit CU key (null in the dev
 * layer), firstBadXcc the CU's XCD, in the dev layer the row's XCD, 8 for the row every workgroup hits. ok = every
 * count 0 and, unless "requireAllCUs":0, cusVerified = CUs; "passed" also needs it. Without the option: no
 * "atomics" key, no launch, allocation or event. Test hooks (any, or the dump below, selects the kernel's test
 * instantiation; all strike wave 0): "injectAtomSkip":[layer, op, step, lane] does not issue that atomic (op 22:
 * the ticket add), (layer 3 in a hook:
 * the lds layer's second addressing), "injectAtomFlip":[layer, op, step, lane, bit] flips one bit of the raw operand (bits to 63 for
 * ops 12..16; for the floating-point ops in the integer, before conversion), "injectAtomFaultXcc":x /
 * "injectAtomFaultWorkgroup":w only on XCD x / in workgroup w; a value out of range switches a hook off.
 *
 * mi355x_probe_atomics: the phase alone, on the device's first stream, under the device's probe lock; the
 * "atomics" block (after "device" and "passed") is the whole report. opts as above (without "atomCheck"). With
 * dump and "atomDumpStage":1|2, workgroup 0's data lands in dump (the first min(dump_bytes, 96256) bytes,
 * uint32): its LDS region [2688] and its lds and l2 digests [4][64] each, as they stood after step 0 (1) or
 * after the last step (2) — the run goes on after a stage-1 dump and is verified in full — then, of the
 * whole run, its private region [2688] and the nine dev row-sets [9][1408] as atom_verify read them, the CU key
 * of every workgroup's record [4096, the first "workgroups" in use; only with the dev layer] and the LDS
 * row-set of the second addressing [1408, the stage's]; the buffer is zeroed first, so what a layer left out
 * of "atomLayers" would have written reads 0. With "atomTimeKernels":1 an event is recorded between the two
 * kernels and the report ends in "marchMs","verifyMs". The report
 * names "dumpCU" and "dumpSimds" as mi355x_probe_regs does. A bad device: {"passed":false,"error":...}. */
char* mi355x_probe_atomics(int device, const char* opts_json, void* dump, size_t dump_bytes);
/* The LDS phase alone, on the device's first stream, under the device's probe lock; the "lds" block (after
 * "device" and "passed") is the whole report. opts as above (without "ldsCheck"). With image and
 * "ldsDumpStage":1|2|3, workgroup 0's LDS is copied out — 1 after the first write, 2 after the first
 * complement write, 3 after the address pass's stores — its first min(image_bytes, tested bytes) land in
 * image and the report names "dumpCU", the CU key that workgroup ran on. A bad device or an "ldsBytes"
 * outside [16, 163840]: {"passed":false,"error":...}. */
char* mi355x_probe_lds(int device, const char* opts_json, void* image, size_t image_bytes);
/* The host-link phase alone, on the device's first stream, under the device's probe lock; the
 * "hostLink" block (after "device" and "passed") is the whole report. opts as above ("hostLinkBytes",
 * "hostLinkPatterns", the hook, the knobs). io may be NULL; after the run the first min(io_bytes, bytes)
 * of the pinned buffer are copied into it. "preload":1 skips the write passes: the first io_bytes of the
 * pinned buffer are loaded from io and one verify of polarity 0 runs over io_bytes / 16 chunks — a pure
 * host -> device check of data the caller made (no host sample, writeGBps 0, GBps = readGBps). A bad
 * device, preload without io, or a size outside [16 B, 4 GiB]: {"passed":false,"error":...}. */
char* mi355x_probe_host_link(int device, const char* opts_json, void* io, size_t io_bytes);
/* The default launch shape of the host-link kernels: workgroups, threads per workgroup, 16-byte
 * accesses per thread and main-loop iteration. One main-loop pass of the whole grid covers
 * grid * threads * unroll chunks. Any pointer may be NULL. */
void mi355x_probe_host_link_geometry(int* grid, int* threads, int* unroll);
/* xGMI peer check: src writes a pattern, copies it to dst over the peer link
 * (hipMemcpyPeerAsync after hipDeviceEnablePeerAccess), dst verifies every bit.
 * opts: {"bytes":268435456} (at least 1 MiB, rounded down to 16). src == dst runs the same path as a
 * local device copy.
 * -> {"src","dst","canAccessPeer":bool,"passed":bool,"badBits","firstBadOffset","bytes","GBps","ms",
 *     "seed"}
 * firstBadOffset: the byte offset of the lowest faulting 16-byte chunk of the destination, or null.
 * seed: what this call filled and verified with — the link's base seed mixed with a per-call nonce
 * (a process-wide counter), so data that an earlier call left in the destination's memory never
 * verifies as this call's. The pattern is the cheap one of the HBM test (pattern16<1>, polarity 0).
 * Test hooks, all on the receiving buffer between the copy and the verify: "injectFlipAtChunk":i
 * (bit 0 of 16-byte chunk i; i >= bytes / 16: no flip), "injectBitFlips":k (0..4096, spread as in
 * mi355x_probe_run); and "skipCopy":1 — the copy is not enqueued, everything else (fill, events,
 * verify) runs, so the check must fail on whatever the destination held. */
char* mi355x_probe_peer(int src, int dst, const char* opts_json);
/* The same check; io may be NULL: after the verify the first min(io_bytes, tested bytes) of the
 * destination buffer are copied into it (what arrived, hooks included). */
char* mi355x_probe_peer_dump(int src, int dst, const char* opts_json, void* io, size_t io_bytes);
/* The whole ring at once: link i copies devs[i] -> devs[(i+1) % n], all links concurrently (each
 * GPU pair of an MI355X node has its own xGMI link), then every receiver verifies. Send / receive
 * windows are kept between calls and freed with the idle arena. A device may repeat ([0, 0] on a
 * 1-GPU box runs local copies through the same path). opts: {"bytes":67108864}
 * -> {"bytes","links":[{"src","dst","canAccessPeer","passed","badBits","firstBadOffset","bytes","GBps",
 *                       "ms","seed"}],"passed":bool}
 * One pattern per source device and call: every link's seed mixes the call's nonce as above, because
 * the kept receive windows still hold the previous ring's data. Test hooks as for mi355x_probe_peer;
 * the two flip hooks strike the receive window of link "injectLink":j (default 0) ahead of that
 * link's verify (links that share a receive window — a repeated device — and are verified after it
 * see the flip too); "skipCopy":1 skips every link's copy. */
char* mi355x_probe_peer_ring(const int* devs, int n, const char* opts_json);
/* One window of the rotating HBM sweep: a buffer of all free HBM minus "reserve" bytes is
 * allocated (kept across calls while "keep" is true; released by mi355x_probe_sweep_release) and
 * [offset, offset+bytes) of it is pattern-tested in both polarities.
 * opts: {"offset":0,"bytes":17179869184,"reserve":4294967296,"keep":false,"injectBitFlips":0}
 * -> {"passed","offset","bytes","span","badBits","firstBadOffset","GBps","ms","allocMs"}
 * offset wraps modulo span and is rounded down to 16; bytes (at least 1 MiB) is clipped to the end of
 * the span and rounded down to 16; both come back as tested. The buffer is made of 1 GiB chunks (the
 * last one shorter): a window that straddles them is tested piece by piece, each piece with a seed of
 * its own. firstBadOffset is a byte offset into the buffer (not into the window), or null. Test hooks,
 * both after the first fill: "injectBitFlips":k (0..4096, spread over the window's first piece),
 * "injectFlipAtChunk":i (bit 0 of the window's 16-byte chunk i, in whichever piece holds it; past the
 * window: no flip). */
char* mi355x_probe_hbm_sweep(int device, const char* opts_json);
/* Allocate / free the sweep buffer without holding the device's probe lock (allocating ~282 GiB
 * takes ~0.4 s and freeing it ~2.9 s on MI355X: a claim-time probe must never wait for either).
 * alloc: 1 = allocated, 0 = already held, <0 = error. Both work in 1 GiB chunks and wait between
 * chunks while a claim-time probe of the device runs. release: 1 = freed, 0 = none held. */
int mi355x_probe_sweep_alloc(int device, long long reserve_bytes);
int mi355x_probe_sweep_release(int device);
/* The probe's production GEMM (256x256x64 MFMA tile) on caller HOST buffers (copied in and out):
 * C[m][n] (fp32) = A[m][k] (bf16, row-major) * Bt[n][k]^T (bf16, row-major). m, n multiples of
 * 256, k of 64. For independent numerics checks against a CPU torch.matmul (torch bundles its own
 * HIP runtime, so device pointers cannot be shared with it in one process). 0 = ok. */
int mi355x_probe_gemm_bf16(int device, const void* A, const void* Bt, void* C, int m, int n, int k);
/* The same on any of the probe's GEMM kernels. opts (JSON or NULL), meanings and defaults as in
 * mi355x_probe_run: "gemmTile" 256 | 128, "gemmPipe" 0 | 1 | 2 | 3 | 21 | 22 (256 only), "gemmPrio",
 * "gemmVecC" (2-phase loop only), "gemmGroupM" (tile order), "poisonC" (the device C is filled with
 * 0xFF bytes before the launch). Tile 256 needs m, n % 256 == 0 and k % 64 == 0; tile 128 m, n % 128
 * == 0 and k % 32 == 0. 0 = ok, -1 bad device, -2 bad arguments (also: an unknown pipe or one of the
 * timing-only ablations 11 / 12), -4 a HIP error. mi355x_probe_gemm_bf16 is this with NULL opts. */
int mi355x_probe_gemm_bf16_opts(int device, const void* A, const void* Bt, void* C, int m, int n, int k,
                                const char* opts_json);
/* The low-precision GEMM of the probe (128x128x128 tile) on caller HOST buffers: C[m][n] (fp32) =
 * A[m][k] * Bt[n][k]^T. dtype 0 fp8, 1 mxfp8 (one e4m3 byte per element), 2 mxfp4 (two e2m1 per byte,
 * even k in the low nibble: rows of k/2 bytes). scaleA / scaleBt: [rows][k/32] E8M0 bytes for the
 * scaled dtypes, NULL for fp8. m, n, k multiples of 128. opts: "poisonC". 0 = ok, -1 bad device,
 * -2 bad arguments (a bad shape, an unknown dtype, scales passed to fp8 or missing for a scaled
 * dtype; C is not touched), -4 a HIP error. */
int mi355x_probe_gemm_lowp(int device, int dtype, const void* A, const void* Bt, const void* scaleA,
                           const void* scaleBt, void* C, int m, int n, int k, const char* opts_json);
/* Test surfaces: the kernels that decide a probe's verdict, on caller HOST buffers, so a test can
 * compare them with a host reference. None of them is on the claim path; each allocates per call,
 * frees on every path and leaves the probe's kept arena alone. dtype: -1 bf16 (2 bytes per element),
 * else the low-precision index of mi355x_probe_gemm_lowp with its operand layouts; scaleA / scaleBt
 * as there (NULL for bf16 and fp8). All return 0 = ok, -1 bad device, -2 bad arguments (no output is
 * touched), -4 a HIP error.
 *
 * abft_check: the probe's ABFT checker sequence (same kernels, grids and order as a probe's) over
 * A[m][k], Bt[n][k] and the caller's C[m][n] (fp32). bf16 needs k % 8 == 0, low precision k % 32 == 0;
 * n % 4 == 0, 1 <= m, n, k <= 65535. bound: the largest |C| the operands allow. vectors: 2k + 2n + 2m
 * words, packed: the column sums of A (k) and of Bt (k), the column sums of C (n) and what they
 * must be (n), the row sums of C (m) and what they must be (m), all mod 2^32. counts[3]: elements
 * of C that are no integer, not finite or beyond the bound; column checksums that differ; row
 * checksums that differ (a probe adds the three into "abftMismatches"). nfaults > 0: after that run,
 * for each i the element fault_index[i] (row * n + col) of the device C is set to fault_value[i], the
 * sequence runs again, the element is put back; fault_counts[3 i ..] are that run's three counts.
 *
 * gemm_ref: the VALU reference of the element check, R[m][n] (fp32) = A * Bt^T, same contract.
 * count_diff: the element check's comparer with its production grid: how many of the count
 * (1 .. 2^31) elements of x and y differ.
 *
 * gen_operands: the in-probe operand generator with its production grid into buffers that start
 * as 0xFF bytes. bf16: count elements of small_int(seed, span = span_or_scale_lo in 1..127) into
 * operand (>= 2 count bytes), and the first nzero words of zero (may be NULL with nzero 0) zeroed;
 * scales NULL. Low precision: count elements (whole 32-bit words) into operand, count / 32 E8M0
 * bytes 2^scale_lo | 2^(scale_lo + 1) into scales for the scaled dtypes (NULL for fp8); nzero 0 and
 * zero NULL. The whole of every buffer (its *_bytes) comes back, so what the generator must not
 * touch still holds 0xFF. */
int mi355x_probe_abft_check(int device, int dtype, const void* A, const void* Bt, const void* scaleA,
                            const void* scaleBt, const void* C, int m, int n, int k, float bound,
                            unsigned int* vectors, unsigned long long* counts, int nfaults,
                            const long long* fault_index, const float* fault_value,
                            unsigned long long* fault_counts);
int mi355x_probe_gemm_ref(int device, int dtype, const void* A, const void* Bt, const void* scaleA,
                          const void* scaleBt, void* R, int m, int n, int k);
int mi355x_probe_count_diff(int device, const float* x, const float* y, unsigned long long count,
                            unsigned long long* bad);
int mi355x_probe_gen_operands(int device, int dtype, unsigned int seed, int span_or_scale_lo,
                              unsigned long long count, unsigned long long nzero, void* operand,
                              size_t operand_bytes, void* scales, size_t scale_bytes, void* zero,
                              size_t zero_bytes);
void mi355x_probe_free(char* p);

#ifdef __cplusplus
}
#endif

#endif /* MI355X_PROBE_H_ */
