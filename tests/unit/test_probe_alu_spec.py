"""spec.probe.aluCheck through the public layers, on the CPU: the schema and the CRD's admission, the
manager's API layer and the probe library's host side (C++), the bindings' option encoding, the agent's
probe plumbing and wording, and the simulated probe."""
from __future__ import annotations

import glob
import json
import os
import subprocess

import pytest
import yaml

from gpupool.agent import simprobe
from gpupool.agent.prober import Prober
from gpupool.apiserver_sim.store import ApiError, Store
from gpupool.ops import probe as hp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
POOLS = ("compute.my.domain", "mi355xpools")
BLOCK_KEYS = ["ok", "iters", "workgroups", "waves", "wavesPerSimd", "simdsTested", "simdsVerified", "cusVerified",
              "perXcd", "badWaves", "badLanes", "badCUs", "firstBadCU", "firstBadSimd", "firstBadGroup", "firstBadLane",
              "splitWaves", "suspectCU", "suspectSimd", "transDigest", "ms"]


@pytest.fixture(scope="module")
def store():
    s = Store()
    crd_rt = s.types[("apiextensions.k8s.io", "customresourcedefinitions")]
    for p in glob.glob(os.path.join(ROOT, "config", "crd", "*.yaml")):
        s.create(crd_rt, None, yaml.safe_load(open(p)))
    return s


def _create(store, name, probe):
    return store.create(store.types[POOLS], "default",
                        {"apiVersion": "compute.my.domain/v1alpha1", "kind": "Mi355xPool",
                         "metadata": {"name": name}, "spec": {"replicas": 1, "probe": probe}})


def test_schema_declares_the_field_and_the_status():
    crd = yaml.safe_load(open(os.path.join(ROOT, "config", "crd", "compute.my.domain_mi355xpools.yaml")))
    root = crd["spec"]["versions"][0]["schema"]["openAPIV3Schema"]["properties"]
    f = root["spec"]["properties"]["probe"]["properties"]["aluCheck"]
    assert f["type"] == "boolean" and f["default"] is False
    for reason in ("ALUResultMismatch", "ALUConsensusSplit", "ALUCoverageShort"):
        assert reason in f["description"]
    st = root["status"]["properties"]["devices"]["items"]["properties"]["probe"]["properties"]
    assert st["aluVerifiedCUs"]["type"] == "integer"
    sample = yaml.safe_load(open(os.path.join(ROOT, "config", "samples", "compute_v1alpha1_mi355xpool_alu.yaml")))
    assert sample["kind"] == "Mi355xPool" and sample["spec"]["probe"]["aluCheck"] is True
    # the low-precision dtype list is what it was: this is a phase of its own
    lowp = root["spec"]["properties"]["probe"]["properties"]["mfmaLowPrecision"]
    assert "alu" not in json.dumps(lowp)


def test_crd_defaults_accepts_and_refuses(store):
    assert _create(store, "d", {})["spec"]["probe"]["aluCheck"] is False
    assert _create(store, "on", {"aluCheck": True})["spec"]["probe"]["aluCheck"] is True
    assert _create(store, "off", {"aluCheck": False, "registerCheck": True})["spec"]["probe"]["aluCheck"] is False
    for bad in ("yes", 1, [True]):
        with pytest.raises(ApiError) as e:
            _create(store, "bad", {"aluCheck": bad})
        assert "aluCheck" in str(e.value.message if hasattr(e.value, "message") else e.value)


def test_native_host_side(native_built):
    """native/tests/test_alu_spec.cc: alu_ref.h against the pinned table, its rounder, the library's options
    and hooks, the "alu" block byte for byte, ok under each failing condition, the unchanged default
    report, and the manager's parse / probe_json / InvalidSpec / aluVerifiedCUs."""
    r = subprocess.run([os.path.join(native_built, "gpupool_tests"), "alu_"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "9 passed, 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def test_run_opts_default_encoding_is_unchanged():
    base = hp._run_opts(1 << 30, True, 4096, 2, 1, 256, ())
    assert base == (b'{"hbmBytes": 1073741824, "mfma": true, "gemmN": 4096, "patterns": 2, "gemmReps": 1, '
                    b'"gemmTile": 256}')
    assert hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 0, False, False) == base
    assert hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 0, False, False, False) == base
    on = json.loads(hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 0, False, False, True))
    assert on == {**json.loads(base), "aluCheck": 1}
    assert list(on)[-1] == "aluCheck"
    every = json.loads(hp._run_opts(1 << 30, True, 2048, 2, 1, 256, (("injectAluFlip", (1, 0, 3, 5)), ("overlap", 1)),
                                    ("fp8",), 1 << 20, True, True, True))
    assert every["aluCheck"] == 1 and every["regCheck"] == 1 and every["ldsCheck"] == 1
    assert every["injectAluFlip"] == [1, 0, 3, 5] and every["overlap"] == 1
    assert list(every).index("ldsCheck") < list(every).index("regCheck") < list(every).index("aluCheck")


def test_run_encodes_the_flag_only_when_asked(monkeypatch):
    seen = []

    class Lib:
        def mi355x_probe_run(self, dev, opts):
            seen.append(json.loads(opts))
            return 1

    monkeypatch.setattr(hp, "lib", lambda: Lib())
    monkeypatch.setattr(hp, "_take", lambda p: {"passed": True})
    hp.run(0, hbm_bytes=1 << 20, gemm_n=512)
    hp.run(0, hbm_bytes=1 << 20, gemm_n=512, alu_check=False)
    hp.run(0, hbm_bytes=1 << 20, gemm_n=512, alu_check=True, aluIters=3, injectAluFlip=[4, 2, 63, 31])
    assert "aluCheck" not in seen[0] and seen[0] == seen[1]
    assert seen[2] == {**seen[0], "aluCheck": 1, "aluIters": 3, "injectAluFlip": [4, 2, 63, 31]}


def test_alu_binding_encodes_options_and_shapes_the_dump(monkeypatch):
    import ctypes

    import numpy as np
    seen = []

    class Lib:
        def mi355x_probe_alu(self, dev, opts, buf, n):
            seen.append((dev, json.loads(opts), n))
            if buf is not None:
                ctypes.memmove(buf, np.arange(4 * 6 * 64, dtype="<u4").tobytes(), n)
            return len(seen)

    monkeypatch.setattr(hp, "lib", lambda: Lib())
    monkeypatch.setattr(hp, "_take", lambda p: {"passed": True, **({"dumpCU": 5} if p == 2 else {})})
    r = hp.alu(3, iters=2, aluBlocksPerCU=8, injectAluFlip=(0, 1, 63, 31))
    assert seen[0] == (3, {"aluIters": 2, "aluBlocksPerCU": 8, "injectAluFlip": [0, 1, 63, 31]}, 0) and "data" not in r
    r = hp.alu(0, want_stage=2)  # the step count is the library's unless given
    assert seen[1] == (0, {"aluDumpStage": 2}, 4 * 6 * 64 * 4)
    assert r["data"].shape == (4, 6, 64) and r["data"].dtype == np.uint32
    assert int(r["data"][1, 2, 3]) == (1 * 6 + 2) * 64 + 3  # wave, group, lane
    r = hp.alu(0, want_stage=1)  # a report without "dumpCU" (an error) carries no dump
    assert "data" not in r


class _Helpers:
    """Stands in for the helper pool: records the args of each call."""

    def __init__(self, res):
        self.calls, self.res = [], res

    def get(self, uuid, dev):
        return self

    def call(self, op, args, timeout):
        self.calls.append((op, args))
        return dict(self.res)


def test_helper_args_carry_the_flag_only_when_asked_for():
    p = Prober("simulated", sim_ms=0)
    p.mode = "helper"
    p.helpers = h = _Helpers({"passed": True})
    dev = {"uuid": "u", "hipUUID": "GPU-0", "index": 0}
    p._one(dev, {})
    p._one(dev, {"aluCheck": False})  # the CRD's default is there, the check is not asked for
    p._one(dev, {"aluCheck": True})
    p._one(dev, {"aluCheck": True, "minHbmGBps": 3000})
    p._one(dev, {"aluCheck": True, "registerCheck": True})
    a = [args for _, args in h.calls]
    assert set(a[0]) == set(a[1]) == {"hipUUID", "hbmBytes", "mfma", "gemmN", "overlap", "hooks"}
    assert a[2]["aluCheck"] is True and set(a[2]) == set(a[0]) | {"aluCheck"}
    assert a[2]["overlap"] == 1 and a[2]["gemmN"] == p.overlap_gemm_n  # the check alone keeps the probe overlapped
    assert a[3]["aluCheck"] is True and a[3]["overlap"] == 0
    assert set(a[4]) == set(a[0]) | {"aluCheck", "registerCheck"}


def test_inproc_and_subprocess_paths_carry_the_flag_only_when_asked_for(monkeypatch):
    class Hip:
        def __init__(self):
            self.kw = []

        def run(self, ordinal, **kw):
            self.kw.append(kw)
            return {"passed": True}

    p = Prober("simulated", sim_ms=0)
    p.mode, p._hip, p.ordinals = "inproc", Hip(), {"gpu-0": 0}
    dev = {"uuid": "u", "hipUUID": "GPU-0", "index": 0}
    p._one(dev, {})
    p._one(dev, {"aluCheck": True})
    assert "alu_check" not in p._hip.kw[0]
    assert p._hip.kw[1] == {**p._hip.kw[0], "alu_check": True}

    cmds = []

    def fake_run(cmd, **kw):
        cmds.append(cmd)
        return subprocess.CompletedProcess(cmd, 0, stdout='{"passed": true}\n', stderr="")

    monkeypatch.setattr("gpupool.agent.prober.subprocess.run", fake_run)
    p.mode = "subprocess"
    p._one(dev, {})
    p._one(dev, {"aluCheck": True})
    p._one(dev, {"aluCheck": True, "registerCheck": True})
    assert "--alu-check" not in cmds[0] and cmds[1] == cmds[0] + ["--alu-check"]
    assert cmds[2] == cmds[0] + ["--register-check", "--alu-check"]


def test_helper_op_passes_the_flag_to_the_binding_only_when_asked():
    from gpupool.agent import probehost

    class Hp:
        def run(self, ordinal, **kw):
            self.kw = kw
            return {"passed": True}

    k = probehost._HipKernel.__new__(probehost._HipKernel)
    k.hp = Hp()
    k.ordinal = lambda uuid: 0
    base = {"hipUUID": "GPU-0", "hbmBytes": 1 << 20, "mfma": True, "gemmN": 512, "overlap": 1}
    k.call("probe", base)
    plain = dict(k.hp.kw)
    assert "alu_check" not in plain
    k.call("probe", {**base, "aluCheck": True})
    assert k.hp.kw == {**plain, "alu_check": True}


def _res(**alu):
    block = {"ok": False, "iters": 32, "workgroups": 256, "waves": 1024, "wavesPerSimd": [256] * 4, "simdsTested": 1024,
             "simdsVerified": 1024, "cusVerified": 256, "perXcd": [128] * 8, "badWaves": 0, "badLanes": 0, "badCUs": 0,
             "firstBadCU": None, "firstBadSimd": None, "firstBadGroup": None, "firstBadLane": None, "splitWaves": 0,
             "suspectCU": None, "suspectSimd": None, "transDigest": "be4719975886aa7e", "ms": 0.07, **alu}
    return {"passed": False, "hbm": {"badBits": 0}, "mfma": {"elementMismatches": 0, "abftMismatches": 0},
            "cus": {"expected": 256, "mfmaVerified": 256, "badWaves": 0, "ok": True}, "alu": block}


def test_explain_wording():
    key = (3 << 8) | (5 << 5) | (1 << 4) | 9  # xcc 3, se 5, sh 1, cu 9
    r = Prober.explain(_res(badWaves=3, badLanes=3, badCUs=2, simdsVerified=1021, cusVerified=254, firstBadCU=key,
                            firstBadSimd=2, firstBadGroup="f64", firstBadLane=63))
    assert r["error"] == "ALUResultMismatch(f64): 3 wave(s) on 2 CU(s), first on CU 3/5/1/9 SIMD 2 lane 63"
    for g in ("int", "f32", "f16", "lane"):
        r = Prober.explain(_res(badWaves=1, badLanes=1, badCUs=1, simdsVerified=1023, firstBadCU=0, firstBadSimd=1,
                                firstBadGroup=g, firstBadLane=7))
        assert r["error"] == f"ALUResultMismatch({g}): 1 wave(s) on 1 CU(s), first on CU 0/0/0/0 SIMD 1 lane 7"
    r = Prober.explain(_res(splitWaves=4, badCUs=1, simdsVerified=1023, cusVerified=255, suspectCU=key, suspectSimd=3))
    assert r["error"] == ("ALUConsensusSplit: 4 of 1024 wave(s) disagree on the transcendental digest, suspect CU "
                          "3/5/1/9 SIMD 3")
    r = Prober.explain(_res(simdsTested=1020, simdsVerified=1020, cusVerified=255))
    assert r["error"] == "ALUCoverageShort: 1020/1024 SIMDs"
    # all three: mismatches and a split on a GPU where not every SIMD was reached
    r = Prober.explain(_res(badWaves=1, badLanes=2, badCUs=2, firstBadCU=1, firstBadSimd=3, firstBadGroup="lane",
                            firstBadLane=4, splitWaves=1, suspectCU=2, suspectSimd=0, simdsTested=1022, simdsVerified=1020))
    assert r["error"] == ("ALUResultMismatch(lane): 1 wave(s) on 2 CU(s), first on CU 0/0/0/1 SIMD 3 lane 4; "
                          "ALUConsensusSplit: 1 of 1024 wave(s) disagree on the transcendental digest, suspect CU 0/0/0/2 "
                          "SIMD 0; ALUCoverageShort: 1020/1024 SIMDs")
    ok = {"passed": True, "alu": {"ok": True, "badWaves": 0}}
    assert Prober.explain(dict(ok)) == ok
    # another block's failure is not put on a clean ALU block
    r = _res(ok=True)
    r["hbm"] = {"badBits": 2, "firstBadOffset": 16}
    assert Prober.explain(r)["error"] == "HBMPatternMismatch: 2 flipped bit(s), first at offset 16"


def test_simulated_probe_reports_the_same_block():
    dev = {"uuid": "u", "index": 3, "asic": {"computeUnits": 256}}
    base = simprobe.probe(dev, {}, 0)
    assert "alu" not in base and "alu" not in simprobe.probe(dev, {"aluCheck": False}, 0)
    r = simprobe.probe(dev, {"aluCheck": True}, 0)
    assert r["passed"] and list(r["alu"]) == BLOCK_KEYS and set(r) - {"alu"} == set(base)
    b = r["alu"]
    assert b["ok"] and b["iters"] == simprobe.SIM_ALU_ITERS
    assert b["workgroups"] == simprobe.SIM_ALU_BLOCKS_PER_CU * 256 and b["waves"] == 4 * b["workgroups"] == sum(b["wavesPerSimd"])
    assert b["simdsTested"] == b["simdsVerified"] == 1024 == sum(b["perXcd"]) and len(b["perXcd"]) == 8
    assert b["cusVerified"] == 256 and b["badWaves"] == b["badLanes"] == b["badCUs"] == b["splitWaves"] == 0
    assert b["firstBadCU"] is b["firstBadSimd"] is b["firstBadGroup"] is b["firstBadLane"] is None
    assert b["suspectCU"] is b["suspectSimd"] is None and len(b["transDigest"]) == 16
    bad = simprobe.probe({**dev, "aluFault": 3}, {"aluCheck": True}, 0)
    b = bad["alu"]
    assert not bad["passed"] and not b["ok"] and bad["hbm"]["ok"] and bad["mfma"]["ok"] and bad["cus"]["ok"]
    assert b["badCUs"] == 3 and b["cusVerified"] == 253 and b["simdsVerified"] == 1012 == sum(b["perXcd"]) and b["simdsTested"] == 1024
    assert b["badWaves"] == b["badLanes"] == 3 * 4 * simprobe.SIM_ALU_BLOCKS_PER_CU
    assert (b["firstBadCU"], b["firstBadSimd"], b["firstBadGroup"], b["firstBadLane"]) == (0, 0, "f32", 0)
    assert Prober.explain(bad)["error"] == \
        f"ALUResultMismatch(f32): {b['badWaves']} wave(s) on 3 CU(s), first on CU 0/0/0/0 SIMD 0 lane 0"
    assert simprobe.probe({**dev, "faults": {"aluFault": 1}}, {"aluCheck": True}, 0)["alu"]["badCUs"] == 1
    assert simprobe.probe({**dev, "aluFault": 3}, {}, 0)["passed"]  # not asked: not run
    assert simprobe.probe({**dev, "aluFault": 3}, {"registerCheck": True}, 0)["passed"]  # another check's overlay
    assert simprobe.probe({**dev, "regFault": 3}, {"aluCheck": True}, 0)["passed"]
    both = simprobe.probe(dev, {"registerCheck": True, "aluCheck": True}, 0)
    assert list(both).index("alu") == list(both).index("regs") + 1
    small = simprobe.probe({"uuid": "p", "asic": {"computeUnits": 32}}, {"aluCheck": True}, 0)["alu"]
    assert small["cusVerified"] == 32 and small["simdsVerified"] == 128 == sum(small["perXcd"])


def test_prober_in_simulated_mode():
    p = Prober("simulated", sim_ms=0)
    dev = {"uuid": "u", "asic": {"computeUnits": 256}}
    assert p.probe_many([dev], {"aluCheck": True})[0]["passed"]
    r = p.probe_many([{**dev, "aluFault": 2}], {"aluCheck": True})[0]
    assert not r["passed"] and r["error"].startswith("ALUResultMismatch(f32): ")
    assert p.probe_many([{**dev, "aluFault": 2}], {})[0]["passed"]


def test_gpuctl_shows_the_verified_cus(capsys):
    from gpupool.cli import gpuctl
    src = open(gpuctl.__file__).read()
    assert 'probe += f" alu {p[\'aluVerifiedCUs\']}CU"' in src
