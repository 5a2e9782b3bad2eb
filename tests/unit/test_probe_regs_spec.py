"""spec.probe.registerCheck through the public layers, on the CPU: the schema and the CRD's admission,
the manager's API layer and the probe library's host side (C++), the bindings' option encoding, the
agent's probe plumbing and wording, and the simulated probe."""
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
BLOCK_KEYS = ["ok", "registersPerLane", "workgroupsPerCU", "patterns", "salt", "workgroups", "cusTested",
              "cusVerified", "simdsTested", "simdShort", "perXcd", "badCUs", "badBits", "firstBadCU",
              "firstBadSimd", "firstBadRegister", "firstBadLane", "ms"]


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
    f = root["spec"]["properties"]["probe"]["properties"]["registerCheck"]
    assert f["type"] == "boolean" and f["default"] is False
    for reason in ("RegisterFileMismatch", "RegisterCoverageShort", "RegisterKernelNotExclusive"):
        assert reason in f["description"]
    st = root["status"]["properties"]["devices"]["items"]["properties"]["probe"]["properties"]
    assert st["regsVerifiedCUs"]["type"] == "integer"
    sample = yaml.safe_load(open(os.path.join(ROOT, "config", "samples", "compute_v1alpha1_mi355xpool_regs.yaml")))
    assert sample["kind"] == "Mi355xPool" and sample["spec"]["probe"]["registerCheck"] is True


def test_crd_defaults_accepts_and_refuses(store):
    assert _create(store, "d", {})["spec"]["probe"]["registerCheck"] is False
    assert _create(store, "on", {"registerCheck": True})["spec"]["probe"]["registerCheck"] is True
    assert _create(store, "off", {"registerCheck": False, "ldsCheck": True})["spec"]["probe"]["registerCheck"] is False
    for bad in ("yes", 1, [True]):
        with pytest.raises(ApiError) as e:
            _create(store, "bad", {"registerCheck": bad})
        assert "registerCheck" in str(e.value.message if hasattr(e.value, "message") else e.value)


def test_native_host_side(native_built):
    """native/tests/test_regs_spec.cc: the library's options and hooks, the "regs" block byte for byte,
    ok under each failing condition, the unchanged default report, and the manager's parse /
    probe_json / InvalidSpec / regsVerifiedCUs."""
    r = subprocess.run([os.path.join(native_built, "gpupool_tests"), "regs_"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "7 passed, 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def test_run_opts_default_encoding_is_unchanged():
    base = hp._run_opts(1 << 30, True, 4096, 2, 1, 256, ())
    assert base == (b'{"hbmBytes": 1073741824, "mfma": true, "gemmN": 4096, "patterns": 2, "gemmReps": 1, '
                    b'"gemmTile": 256}')
    assert hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 0, False) == base
    assert hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 0, False, False) == base
    on = json.loads(hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 0, False, True))
    assert on == {**json.loads(base), "regCheck": 1}
    assert list(on)[-1] == "regCheck"
    every = json.loads(hp._run_opts(1 << 30, True, 2048, 2, 1, 256, (("injectRegFlip", (17, 3, 5)), ("overlap", 1)),
                                    ("fp8",), 1 << 20, True, True))
    assert every["regCheck"] == 1 and every["ldsCheck"] == 1 and every["hostLinkBytes"] == 1 << 20
    assert every["injectRegFlip"] == [17, 3, 5] and every["overlap"] == 1
    assert list(every).index("ldsCheck") < list(every).index("regCheck")


def test_run_encodes_the_flag_only_when_asked(monkeypatch):
    seen = []

    class Lib:
        def mi355x_probe_run(self, dev, opts):
            seen.append(json.loads(opts))
            return 1

    monkeypatch.setattr(hp, "lib", lambda: Lib())
    monkeypatch.setattr(hp, "_take", lambda p: {"passed": True})
    hp.run(0, hbm_bytes=1 << 20, gemm_n=512)
    hp.run(0, hbm_bytes=1 << 20, gemm_n=512, reg_check=False)
    hp.run(0, hbm_bytes=1 << 20, gemm_n=512, reg_check=True, regsBlocksPerCU=2, injectRegFlip=[300, 1, 31])
    assert "regCheck" not in seen[0] and seen[0] == seen[1]
    assert seen[2] == {**seen[0], "regCheck": 1, "regsBlocksPerCU": 2, "injectRegFlip": [300, 1, 31]}


def test_regs_binding_encodes_options_and_shapes_the_image(monkeypatch):
    import ctypes

    import numpy as np
    seen = []

    class Lib:
        def mi355x_probe_regs(self, dev, opts, buf, n):
            seen.append((dev, json.loads(opts), n))
            if buf is not None:
                ctypes.memmove(buf, np.arange(4 * 512 * 64, dtype="<u4").tobytes(), n)
            return len(seen)

    monkeypatch.setattr(hp, "lib", lambda: Lib())
    monkeypatch.setattr(hp, "_take", lambda p: {"passed": True, **({"dumpCU": 5} if p == 2 else {})})
    r = hp.regs(3, patterns=1, regsBlocksPerCU=8, injectRegFlip=(0, 63, 31))
    assert seen[0] == (3, {"regsPatterns": 1, "regsBlocksPerCU": 8, "injectRegFlip": [0, 63, 31]}, 0) and "data" not in r
    r = hp.regs(0, want_stage=2)
    assert seen[1] == (0, {"regsPatterns": 2, "regsDumpStage": 2}, 4 * 512 * 64 * 4)
    assert r["data"].shape == (4, 512, 64) and r["data"].dtype == np.uint32
    assert int(r["data"][1, 2, 3]) == (1 * 512 + 2) * 64 + 3  # wave, register, lane
    r = hp.regs(0, want_stage=1)  # a report without "dumpCU" (an error) carries no image
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
    p._one(dev, {"registerCheck": False})  # the CRD's default is there, the check is not asked for
    p._one(dev, {"registerCheck": True})
    p._one(dev, {"registerCheck": True, "minHbmGBps": 3000})
    p._one(dev, {"registerCheck": True, "ldsCheck": True})
    a = [args for _, args in h.calls]
    assert set(a[0]) == set(a[1]) == {"hipUUID", "hbmBytes", "mfma", "gemmN", "overlap", "hooks"}
    assert a[2]["registerCheck"] is True and set(a[2]) == set(a[0]) | {"registerCheck"}
    assert a[2]["overlap"] == 1 and a[2]["gemmN"] == p.overlap_gemm_n  # the check alone keeps the probe overlapped
    assert a[3]["registerCheck"] is True and a[3]["overlap"] == 0
    assert set(a[4]) == set(a[0]) | {"registerCheck", "ldsCheck"}


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
    p._one(dev, {"registerCheck": True})
    assert "reg_check" not in p._hip.kw[0]
    assert p._hip.kw[1] == {**p._hip.kw[0], "reg_check": True}

    cmds = []

    def fake_run(cmd, **kw):
        cmds.append(cmd)
        return subprocess.CompletedProcess(cmd, 0, stdout='{"passed": true}\n', stderr="")

    monkeypatch.setattr("gpupool.agent.prober.subprocess.run", fake_run)
    p.mode = "subprocess"
    p._one(dev, {})
    p._one(dev, {"registerCheck": True})
    p._one(dev, {"registerCheck": True, "ldsCheck": True})
    assert "--register-check" not in cmds[0] and cmds[1] == cmds[0] + ["--register-check"]
    assert cmds[2] == cmds[0] + ["--lds-check", "--register-check"]


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
    assert "reg_check" not in plain
    k.call("probe", {**base, "registerCheck": True})
    assert k.hp.kw == {**plain, "reg_check": True}


def _res(**regs):
    block = {"ok": False, "registersPerLane": 512, "workgroupsPerCU": 1, "patterns": 2, "salt": 0, "workgroups": 512,
             "cusTested": 256, "cusVerified": 256, "simdsTested": 1024, "simdShort": 0, "perXcd": [32] * 8,
             "badCUs": 0, "badBits": 0, "firstBadCU": None, "firstBadSimd": None, "firstBadRegister": None,
             "firstBadLane": None, "ms": 0.15, **regs}
    return {"passed": False, "hbm": {"badBits": 0}, "mfma": {"elementMismatches": 0, "abftMismatches": 0},
            "cus": {"expected": 256, "mfmaVerified": 256, "badWaves": 0, "ok": True}, "regs": block}


def test_explain_wording():
    key = (3 << 8) | (5 << 5) | (1 << 4) | 9  # xcc 3, se 5, sh 1, cu 9
    r = Prober.explain(_res(badBits=3, badCUs=2, cusVerified=254, firstBadCU=key, firstBadSimd=2,
                            firstBadRegister=17, firstBadLane=63))
    assert r["error"] == ("RegisterFileMismatch: 3 flipped bit(s) on 2 CU(s), first on CU 3/5/1/9 SIMD 2 "
                          "register v17 lane 63")
    r = Prober.explain(_res(badBits=1, badCUs=1, cusVerified=255, firstBadCU=0, firstBadSimd=0,
                            firstBadRegister=259, firstBadLane=0))
    assert r["error"] == "RegisterFileMismatch: 1 flipped bit(s) on 1 CU(s), first on CU 0/0/0/0 SIMD 0 register a3 lane 0"
    for u, name in ((0, "v0"), (255, "v255"), (256, "a0"), (511, "a255")):
        r = Prober.explain(_res(badBits=1, badCUs=1, firstBadCU=0, firstBadSimd=1, firstBadRegister=u, firstBadLane=7))
        assert f" SIMD 1 register {name} lane 7" in r["error"], r["error"]
    per = [32, 32, 32, 30, 32, 32, 32, 32]
    r = Prober.explain(_res(cusTested=254, cusVerified=254, perXcd=per))
    assert r["error"] == (f"RegisterCoverageShort: 254/256 CUs verified, per XCD {per}, 0 workgroup(s) on fewer "
                          "than 4 SIMDs")
    r = Prober.explain(_res(cusTested=255, cusVerified=255, perXcd=per, simdShort=2))
    assert r["error"].startswith("RegisterCoverageShort: 255/256 CUs verified") and \
        r["error"].endswith("2 workgroup(s) on fewer than 4 SIMDs")
    # both: a bad bit on a GPU where not every CU was reached
    r = Prober.explain(_res(badBits=1, badCUs=1, cusTested=254, cusVerified=253, firstBadCU=1, firstBadSimd=3,
                            firstBadRegister=16, firstBadLane=4, perXcd=per))
    assert r["error"].startswith("RegisterFileMismatch: 1 flipped bit(s) on 1 CU(s), first on CU 0/0/0/1 SIMD 3 "
                                 "register v16 lane 4; RegisterCoverageShort: 253/256 CUs verified")
    # a kernel that did not own its CU
    r = Prober.explain(_res(registersPerLane=256, workgroupsPerCU=2))
    assert r["error"] == "RegisterKernelNotExclusive: 256 registers per lane, 2 workgroup(s) per CU"
    ok = {"passed": True, "regs": {"ok": True, "badBits": 0}}
    assert Prober.explain(dict(ok)) == ok
    # another block's failure is not put on a clean register block
    r = _res(ok=True)
    r["hbm"] = {"badBits": 2, "firstBadOffset": 16}
    assert Prober.explain(r)["error"] == "HBMPatternMismatch: 2 flipped bit(s), first at offset 16"


def test_simulated_probe_reports_the_same_block():
    dev = {"uuid": "u", "index": 3, "asic": {"computeUnits": 256}}
    base = simprobe.probe(dev, {}, 0)
    assert "regs" not in base and "regs" not in simprobe.probe(dev, {"registerCheck": False}, 0)
    r = simprobe.probe(dev, {"registerCheck": True}, 0)
    assert r["passed"] and list(r["regs"]) == BLOCK_KEYS and set(r) - {"regs"} == set(base)
    b = r["regs"]
    assert b["ok"] and b["registersPerLane"] == 512 and b["workgroupsPerCU"] == 1 and b["patterns"] == 2
    assert b["cusTested"] == b["cusVerified"] == 256 == sum(b["perXcd"]) and len(b["perXcd"]) == 8
    assert b["simdsTested"] == 4 * b["cusTested"] and b["simdShort"] == 0
    assert b["workgroups"] == simprobe.SIM_REGS_BLOCKS_PER_CU * 256
    assert b["badCUs"] == b["badBits"] == 0
    assert b["firstBadCU"] is b["firstBadSimd"] is b["firstBadRegister"] is b["firstBadLane"] is None
    bad = simprobe.probe({**dev, "regFault": 3}, {"registerCheck": True}, 0)
    b = bad["regs"]
    assert not bad["passed"] and not b["ok"] and bad["hbm"]["ok"] and bad["mfma"]["ok"] and bad["cus"]["ok"]
    assert b["badCUs"] == b["badBits"] == 3 and b["cusVerified"] == 253 == sum(b["perXcd"]) and b["cusTested"] == 256
    assert (b["firstBadCU"], b["firstBadSimd"], b["firstBadRegister"], b["firstBadLane"]) == (0, 0, 17, 0)
    assert Prober.explain(bad)["error"] == \
        "RegisterFileMismatch: 3 flipped bit(s) on 3 CU(s), first on CU 0/0/0/0 SIMD 0 register v17 lane 0"
    assert simprobe.probe({**dev, "faults": {"regFault": 1}}, {"registerCheck": True}, 0)["regs"]["badCUs"] == 1
    assert simprobe.probe({**dev, "regFault": 3}, {}, 0)["passed"]  # not asked: not run
    assert simprobe.probe({**dev, "regFault": 3}, {"ldsCheck": True}, 0)["passed"]  # another check's overlay
    both = simprobe.probe(dev, {"ldsCheck": True, "registerCheck": True}, 0)
    assert list(both).index("regs") == list(both).index("lds") + 1
    small = simprobe.probe({"uuid": "p", "asic": {"computeUnits": 32}}, {"registerCheck": True}, 0)["regs"]
    assert small["cusVerified"] == 32 == sum(small["perXcd"])


def test_prober_in_simulated_mode():
    p = Prober("simulated", sim_ms=0)
    dev = {"uuid": "u", "asic": {"computeUnits": 256}}
    assert p.probe_many([dev], {"registerCheck": True})[0]["passed"]
    r = p.probe_many([{**dev, "regFault": 2}], {"registerCheck": True})[0]
    assert not r["passed"] and r["error"].startswith("RegisterFileMismatch: 2 flipped bit(s) on 2 CU(s)")
    assert p.probe_many([{**dev, "regFault": 2}], {})[0]["passed"]
