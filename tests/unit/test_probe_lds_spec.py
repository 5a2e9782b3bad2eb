"""spec.probe.ldsCheck through the public layers, on the CPU: the schema and the CRD's admission, the
manager's API layer and the probe library's host side (C++), the bindings' option encoding, the
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
BLOCK_KEYS = ["ok", "bytesPerCU", "patterns", "salt", "workgroups", "cusTested", "cusVerified", "perXcd",
              "badCUs", "badBits", "firstBadCU", "firstBadOffset", "ms"]


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
    f = root["spec"]["properties"]["probe"]["properties"]["ldsCheck"]
    assert f["type"] == "boolean" and f["default"] is False
    assert "LDSPatternMismatch" in f["description"] and "LDSCoverageShort" in f["description"]
    st = root["status"]["properties"]["devices"]["items"]["properties"]["probe"]["properties"]
    assert st["ldsVerifiedCUs"]["type"] == "integer"


def test_crd_defaults_accepts_and_refuses(store):
    assert _create(store, "d", {})["spec"]["probe"]["ldsCheck"] is False
    assert _create(store, "on", {"ldsCheck": True})["spec"]["probe"]["ldsCheck"] is True
    assert _create(store, "off", {"ldsCheck": False, "hostLinkCheck": True})["spec"]["probe"]["ldsCheck"] is False
    for bad in ("yes", 1, [True]):
        with pytest.raises(ApiError) as e:
            _create(store, "bad", {"ldsCheck": bad})
        assert "ldsCheck" in str(e.value.message if hasattr(e.value, "message") else e.value)


def test_native_host_side(native_built):
    """native/tests/test_lds_spec.cc: the library's options and stride, the "lds" block byte for byte,
    the unchanged default report, and the manager's parse / probe_json / InvalidSpec / ldsVerifiedCUs."""
    r = subprocess.run([os.path.join(native_built, "gpupool_tests"), "lds_"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "6 passed, 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def test_run_opts_default_encoding_is_unchanged():
    base = hp._run_opts(1 << 30, True, 4096, 2, 1, 256, ())
    assert base == (b'{"hbmBytes": 1073741824, "mfma": true, "gemmN": 4096, "patterns": 2, "gemmReps": 1, '
                    b'"gemmTile": 256}')
    assert hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 0) == base
    assert hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 0, False) == base
    on = json.loads(hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 0, True))
    assert on == {**json.loads(base), "ldsCheck": 1}
    assert list(on)[-1] == "ldsCheck"
    every = json.loads(hp._run_opts(1 << 30, True, 2048, 2, 1, 256, (("injectLdsFlipAtByte", 7), ("overlap", 1)),
                                    ("fp8",), 1 << 20, True))
    assert every["ldsCheck"] == 1 and every["hostLinkBytes"] == 1 << 20 and every["mfmaLowPrecision"] == 1
    assert every["injectLdsFlipAtByte"] == 7 and every["overlap"] == 1


def test_run_encodes_the_flag_only_when_asked(monkeypatch):
    seen = []

    class Lib:
        def mi355x_probe_run(self, dev, opts):
            seen.append(json.loads(opts))
            return 1

    monkeypatch.setattr(hp, "lib", lambda: Lib())
    monkeypatch.setattr(hp, "_take", lambda p: {"passed": True})
    hp.run(0, hbm_bytes=1 << 20, gemm_n=512)
    hp.run(0, hbm_bytes=1 << 20, gemm_n=512, lds_check=False)
    hp.run(0, hbm_bytes=1 << 20, gemm_n=512, lds_check=True, ldsBlocksPerCU=2)
    assert "ldsCheck" not in seen[0] and seen[0] == seen[1]
    assert seen[2] == {**seen[0], "ldsCheck": 1, "ldsBlocksPerCU": 2}


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
    p._one(dev, {"ldsCheck": False})  # the CRD's default is there, the check is not asked for
    p._one(dev, {"ldsCheck": True})
    p._one(dev, {"ldsCheck": True, "minHbmGBps": 3000})
    a = [args for _, args in h.calls]
    assert set(a[0]) == set(a[1]) == {"hipUUID", "hbmBytes", "mfma", "gemmN", "overlap", "hooks"}
    assert a[2]["ldsCheck"] is True and set(a[2]) == set(a[0]) | {"ldsCheck"}
    assert a[2]["overlap"] == 1 and a[2]["gemmN"] == p.overlap_gemm_n  # the check alone keeps the probe overlapped
    assert a[3]["ldsCheck"] is True and a[3]["overlap"] == 0


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
    p._one(dev, {"ldsCheck": True})
    assert "lds_check" not in p._hip.kw[0]
    assert p._hip.kw[1] == {**p._hip.kw[0], "lds_check": True}

    cmds = []

    def fake_run(cmd, **kw):
        cmds.append(cmd)
        return subprocess.CompletedProcess(cmd, 0, stdout='{"passed": true}\n', stderr="")

    monkeypatch.setattr("gpupool.agent.prober.subprocess.run", fake_run)
    p.mode = "subprocess"
    p._one(dev, {})
    p._one(dev, {"ldsCheck": True})
    assert "--lds-check" not in cmds[0] and cmds[1] == cmds[0] + ["--lds-check"]


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
    assert "lds_check" not in plain
    k.call("probe", {**base, "ldsCheck": True})
    assert k.hp.kw == {**plain, "lds_check": True}


def _res(**lds):
    block = {"ok": False, "bytesPerCU": 163840, "patterns": 2, "salt": 0, "workgroups": 1024, "cusTested": 256,
             "cusVerified": 256, "perXcd": [32] * 8, "badCUs": 0, "badBits": 0, "firstBadCU": None,
             "firstBadOffset": None, "ms": 0.2, **lds}
    return {"passed": False, "hbm": {"badBits": 0}, "mfma": {"elementMismatches": 0, "abftMismatches": 0},
            "cus": {"expected": 256, "mfmaVerified": 256, "badWaves": 0, "ok": True}, "lds": block}


def test_explain_wording():
    key = (3 << 8) | (5 << 5) | (1 << 4) | 9  # xcc 3, se 5, sh 1, cu 9
    r = Prober.explain(_res(badBits=3, badCUs=2, cusVerified=254, firstBadCU=key, firstBadOffset=163839))
    assert r["error"] == "LDSPatternMismatch: 3 flipped bit(s) on 2 CU(s), first on CU 3/5/1/9 at LDS offset 163839"
    r = Prober.explain(_res(badBits=1, badCUs=1, cusVerified=255, firstBadCU=0, firstBadOffset=0))
    assert r["error"] == "LDSPatternMismatch: 1 flipped bit(s) on 1 CU(s), first on CU 0/0/0/0 at LDS offset 0"
    per = [32, 32, 32, 30, 32, 32, 32, 32]
    r = Prober.explain(_res(cusTested=254, cusVerified=254, perXcd=per))
    assert r["error"] == f"LDSCoverageShort: 254/256 CUs verified, per XCD {per}"
    # both: a bad bit on a GPU where not every CU was reached
    r = Prober.explain(_res(badBits=1, badCUs=1, cusTested=254, cusVerified=253, firstBadCU=1, firstBadOffset=4, perXcd=per))
    assert r["error"] == ("LDSPatternMismatch: 1 flipped bit(s) on 1 CU(s), first on CU 0/0/0/1 at LDS offset 4; "
                          f"LDSCoverageShort: 253/256 CUs verified, per XCD {per}")
    ok = {"passed": True, "lds": {"ok": True, "badBits": 0}}
    assert Prober.explain(dict(ok)) == ok
    # another block's failure is not put on a clean LDS block
    r = _res(ok=True)
    r["hbm"] = {"badBits": 2, "firstBadOffset": 16}
    assert Prober.explain(r)["error"] == "HBMPatternMismatch: 2 flipped bit(s), first at offset 16"


def test_simulated_probe_reports_the_same_block():
    dev = {"uuid": "u", "index": 3, "asic": {"computeUnits": 256}}
    base = simprobe.probe(dev, {}, 0)
    assert "lds" not in base and "lds" not in simprobe.probe(dev, {"ldsCheck": False}, 0)
    r = simprobe.probe(dev, {"ldsCheck": True}, 0)
    assert r["passed"] and list(r["lds"]) == BLOCK_KEYS and set(r) - {"lds"} == set(base)
    b = r["lds"]
    assert b["ok"] and b["bytesPerCU"] == 163840 and b["patterns"] == 2
    assert b["cusTested"] == b["cusVerified"] == 256 == sum(b["perXcd"]) and len(b["perXcd"]) == 8
    assert b["workgroups"] == simprobe.SIM_LDS_BLOCKS_PER_CU * 256
    assert b["badCUs"] == b["badBits"] == 0 and b["firstBadCU"] is None and b["firstBadOffset"] is None
    bad = simprobe.probe({**dev, "ldsFault": 3}, {"ldsCheck": True}, 0)
    b = bad["lds"]
    assert not bad["passed"] and not b["ok"] and bad["hbm"]["ok"] and bad["mfma"]["ok"] and bad["cus"]["ok"]
    assert b["badCUs"] == b["badBits"] == 3 and b["cusVerified"] == 253 == sum(b["perXcd"]) and b["cusTested"] == 256
    assert b["firstBadCU"] == 0 and b["firstBadOffset"] == 0
    assert Prober.explain(bad)["error"] == \
        "LDSPatternMismatch: 3 flipped bit(s) on 3 CU(s), first on CU 0/0/0/0 at LDS offset 0"
    assert simprobe.probe({**dev, "faults": {"ldsFault": 1}}, {"ldsCheck": True}, 0)["lds"]["badCUs"] == 1
    assert simprobe.probe({**dev, "ldsFault": 3}, {}, 0)["passed"]  # not asked: not run
    small = simprobe.probe({"uuid": "p", "asic": {"computeUnits": 32}}, {"ldsCheck": True}, 0)["lds"]
    assert small["cusVerified"] == 32 == sum(small["perXcd"])


def test_prober_in_simulated_mode():
    p = Prober("simulated", sim_ms=0)
    dev = {"uuid": "u", "asic": {"computeUnits": 256}}
    assert p.probe_many([dev], {"ldsCheck": True})[0]["passed"]
    r = p.probe_many([{**dev, "ldsFault": 2}], {"ldsCheck": True})[0]
    assert not r["passed"] and r["error"].startswith("LDSPatternMismatch: 2 flipped bit(s) on 2 CU(s)")
    assert p.probe_many([{**dev, "ldsFault": 2}], {})[0]["passed"]
