"""spec.probe.atomicsCheck from the CRD to the probe library's options: schema, CRD and OpenAPI carry the
field, the prober, the helper and the CLI path pass it through only when asked for, the binding encodes
the phase's options and shapes the dump, the failure reasons read as documented and the simulated probe's
block has the library's key order."""
from __future__ import annotations

import glob
import json
import os
import subprocess

import pytest
import yaml

from gpupool.agent import simprobe
from gpupool.agent.prober import Prober
from gpupool.api import schema
from gpupool.apiserver_sim.store import ApiError, Store
from gpupool.ops import atomics as twin
from gpupool.ops import probe as hp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
POOLS = ("compute.my.domain", "mi355xpools")
BLOCK_KEYS = ["ok", "iters", "layers", "workgroups", "wgPerXcd", "cusTested", "cusVerified", "perXcd", "badCUs",
              "badWorkgroups", "ldsBadSlots", "l2BadSlots", "devBadSlots", "badReturns", "ticketFaults", "firstBadCU",
              "firstBadLayer", "firstBadOp", "firstBadSlot", "firstBadXcc", "ms"]


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
    f = root["spec"]["properties"]["probe"]["properties"]["atomicsCheck"]
    assert f["type"] == "boolean" and f["default"] is False
    for reason in ("AtomicResultMismatch", "AtomicCoverageShort"):
        assert reason in f["description"]
    st = root["status"]["properties"]["devices"]["items"]["properties"]["probe"]["properties"]
    assert st["atomicsVerifiedCUs"]["type"] == "integer"
    # the Python schema the manifests are generated from says the same
    assert schema.MI355X_SPEC["properties"]["probe"]["properties"]["atomicsCheck"]["default"] is False
    assert "atomicsVerifiedCUs" in schema.DEVICE_STATUS["properties"]["probe"]["properties"]
    sample = yaml.safe_load(open(os.path.join(ROOT, "config", "samples", "compute_v1alpha1_mi355xpool_atomics.yaml")))
    assert sample["kind"] == "Mi355xPool" and sample["spec"]["probe"]["atomicsCheck"] is True
    r = subprocess.run(["python", os.path.join(ROOT, "scripts", "gen_manifests.py"), "--check"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_crd_defaults_accepts_and_refuses(store):
    assert _create(store, "d", {})["spec"]["probe"]["atomicsCheck"] is False
    assert _create(store, "on", {"atomicsCheck": True})["spec"]["probe"]["atomicsCheck"] is True
    assert _create(store, "off", {"atomicsCheck": False, "aluCheck": True})["spec"]["probe"]["atomicsCheck"] is False
    for bad in ("yes", 1, [True]):
        with pytest.raises(ApiError) as e:
            _create(store, "bad", {"atomicsCheck": bad})
        assert "atomicsCheck" in str(e.value.message if hasattr(e.value, "message") else e.value)


def test_native_host_side(native_built):
    """native/tests/test_atomics_spec.cc: atomics_ref.h against the pinned table, the exactness bound, the
    library's options and hooks, the "atomics" block byte for byte, ok under each failing condition, the
    unchanged default report, and the manager's parse / probe_json / InvalidSpec / atomicsVerifiedCUs."""
    r = subprocess.run([os.path.join(native_built, "gpupool_tests"), "atomics_"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "10 passed, 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def test_run_opts_default_encoding_is_unchanged():
    base = hp._run_opts(1 << 30, True, 4096, 2, 1, 256, ())
    assert base == (b'{"hbmBytes": 1073741824, "mfma": true, "gemmN": 4096, "patterns": 2, "gemmReps": 1, '
                    b'"gemmTile": 256}')
    assert hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 0, False, False, False, False) == base
    on = json.loads(hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 0, False, False, False, True))
    assert on == {**json.loads(base), "atomCheck": 1} and list(on)[-1] == "atomCheck"
    both = json.loads(hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 0, False, False, True, True))
    assert list(both).index("aluCheck") < list(both).index("atomCheck")


def test_run_encodes_the_flag_only_when_asked(monkeypatch):
    seen = []

    class Lib:
        def mi355x_probe_run(self, dev, opts):
            seen.append(json.loads(opts))
            return 1

    monkeypatch.setattr(hp, "lib", lambda: Lib())
    monkeypatch.setattr(hp, "_take", lambda p: {"passed": True})
    hp.run(0, hbm_bytes=1 << 20, gemm_n=512)
    hp.run(0, hbm_bytes=1 << 20, gemm_n=512, atom_check=False)
    hp.run(0, hbm_bytes=1 << 20, gemm_n=512, atom_check=True, atomIters=3, injectAtomFlip=[2, 12, 0, 63, 63])
    hp.run(0, hbm_bytes=1 << 20, gemm_n=512, alu_check=True)
    assert "atomCheck" not in seen[0] and seen[0] == seen[1]
    assert seen[2] == {**seen[0], "atomCheck": 1, "atomIters": 3, "injectAtomFlip": [2, 12, 0, 63, 63]}
    assert seen[3] == {**seen[0], "aluCheck": 1}


def test_atomics_binding_encodes_options_and_shapes_the_dump(monkeypatch):
    import ctypes

    import numpy as np
    seen = []

    class Lib:
        def mi355x_probe_atomics(self, dev, opts, buf, n):
            seen.append((dev, json.loads(opts), n))
            if buf is not None:
                ctypes.memmove(buf, np.arange(twin.DUMP_WORDS, dtype="<u4").tobytes(), n)
            return len(seen)

    monkeypatch.setattr(hp, "lib", lambda: Lib())
    monkeypatch.setattr(hp, "_take", lambda p: {"passed": True, **({"dumpCU": 5, "workgroups": 768} if p == 2 else {})})
    r = hp.atomics(3, iters=2, atomBlocksPerCU=3, injectAtomSkip=(0, 22, 0, 63))
    assert seen[0] == (3, {"atomIters": 2, "atomBlocksPerCU": 3, "injectAtomSkip": [0, 22, 0, 63]}, 0) and "region" not in r
    r = hp.atomics(0, want_stage=2)  # the step count is the library's unless given
    assert seen[1] == (0, {"atomDumpStage": 2}, 96256)
    assert r["ldsTable"].shape == (2688,) and r["ldsDigests"].shape == r["l2Digests"].shape == (4, 64)
    assert r["region"].shape == (2688,) and r["devRows"].shape == (9, 1408) and len(r["wgXcc"]) == 768
    assert r["ldsTable16"].shape == (1408,) and int(r["ldsTable16"][0]) == twin.DUMP_LDS16
    assert int(r["ldsDigests"][1, 2]) == 2688 + 64 + 2 and int(r["region"][0]) == 2688 + 512
    assert int(r["devRows"][8, 1407]) == 2 * 2688 + 512 + 9 * 1408 - 1 and r["wgKeys"][0] == 2 * 2688 + 512 + 9 * 1408
    assert "region" not in hp.atomics(0, want_stage=1)  # a report without "dumpCU" (an error) carries no dump


class _Helpers:
    """Stands in for the helper pool: records the args of each call."""

    def __init__(self, res):
        self.calls, self.res = [], res

    def get(self, uuid, dev):
        return self

    def call(self, op, args, timeout):
        self.calls.append((op, args))
        return dict(self.res)


def test_every_probe_path_carries_the_flag_only_when_asked_for(monkeypatch):
    p = Prober("simulated", sim_ms=0)
    p.mode = "helper"
    p.helpers = h = _Helpers({"passed": True})
    dev = {"uuid": "u", "hipUUID": "GPU-0", "index": 0}
    p._one(dev, {})
    p._one(dev, {"atomicsCheck": False})  # the CRD's default is there, the check is not asked for
    p._one(dev, {"atomicsCheck": True})
    p._one(dev, {"atomicsCheck": True, "aluCheck": True})
    a = [args for _, args in h.calls]
    assert set(a[0]) == set(a[1]) == {"hipUUID", "hbmBytes", "mfma", "gemmN", "overlap", "hooks"}
    assert a[2]["atomicsCheck"] is True and set(a[2]) == set(a[0]) | {"atomicsCheck"} and a[2]["overlap"] == 1
    assert set(a[3]) == set(a[0]) | {"atomicsCheck", "aluCheck"}

    class Hip:
        def __init__(self):
            self.kw = []

        def run(self, ordinal, **kw):
            self.kw.append(kw)
            return {"passed": True}

    p.mode, p._hip, p.ordinals = "inproc", Hip(), {"gpu-0": 0}
    p._one(dev, {})
    p._one(dev, {"atomicsCheck": True})
    assert "atom_check" not in p._hip.kw[0] and p._hip.kw[1] == {**p._hip.kw[0], "atom_check": True}

    cmds = []

    def fake_run(cmd, **kw):
        cmds.append(cmd)
        return subprocess.CompletedProcess(cmd, 0, stdout='{"passed": true}\n', stderr="")

    monkeypatch.setattr("gpupool.agent.prober.subprocess.run", fake_run)
    p.mode = "subprocess"
    p._one(dev, {})
    p._one(dev, {"atomicsCheck": True})
    p._one(dev, {"atomicsCheck": True, "aluCheck": True})
    assert "--atomics-check" not in cmds[0] and cmds[1] == cmds[0] + ["--atomics-check"]
    assert cmds[2] == cmds[0] + ["--alu-check", "--atomics-check"]

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
    assert "atom_check" not in plain
    k.call("probe", {**base, "atomicsCheck": True})
    assert k.hp.kw == {**plain, "atom_check": True}


def _res(**atom):
    block = {"ok": False, "iters": 1, "layers": 7, "workgroups": 256, "wgPerXcd": [32] * 8, "cusTested": 256,
             "cusVerified": 256, "perXcd": [32] * 8, "badCUs": 0, "badWorkgroups": 0, "ldsBadSlots": 0, "l2BadSlots": 0,
             "devBadSlots": 0, "badReturns": 0, "ticketFaults": 0, "firstBadCU": None, "firstBadLayer": None,
             "firstBadOp": None, "firstBadSlot": None, "firstBadXcc": None, "ms": 0.05, **atom}
    return {"passed": False, "hbm": {"badBits": 0}, "mfma": {"elementMismatches": 0, "abftMismatches": 0},
            "cus": {"expected": 256, "mfmaVerified": 256, "badWaves": 0, "ok": True}, "atomics": block}


def test_explain_wording():
    key = (3 << 8) | (5 << 5) | (1 << 4) | 9  # xcc 3, se 5, sh 1, cu 9
    r = Prober.explain(_res(ldsBadSlots=2, badReturns=1, badCUs=2, badWorkgroups=2, cusVerified=254, firstBadCU=key,
                            firstBadLayer="lds", firstBadOp="xor", firstBadSlot=31, firstBadXcc=3))
    assert r["error"] == "AtomicResultMismatch(lds/xor): 3 slot(s) on 2 CU(s), first on CU 3/5/1/9 slot 31"
    r = Prober.explain(_res(l2BadSlots=1, badCUs=1, badWorkgroups=1, cusVerified=255, firstBadCU=0, firstBadLayer="l2",
                            firstBadOp="cas", firstBadSlot=255, firstBadXcc=0))
    assert r["error"] == "AtomicResultMismatch(l2/cas): 1 slot(s) on 1 CU(s), first on CU 0/0/0/0 slot 255"
    r = Prober.explain(_res(devBadSlots=2, firstBadLayer="dev", firstBadOp="add_f32", firstBadSlot=7, firstBadXcc=8))
    assert r["error"] == "AtomicResultMismatch(dev/add_f32): 2 slot(s) on 0 CU(s), first in the all-XCD row slot 7"
    r = Prober.explain(_res(devBadSlots=1, firstBadLayer="dev", firstBadOp="or", firstBadSlot=0, firstBadXcc=5))
    assert r["error"] == "AtomicResultMismatch(dev/or): 1 slot(s) on 0 CU(s), first in the XCD 5 row slot 0"
    r = Prober.explain(_res(cusTested=250, cusVerified=250, perXcd=[32, 32, 32, 32, 32, 32, 32, 26]))
    assert r["error"] == "AtomicCoverageShort: 250/256 CUs verified, per XCD [32, 32, 32, 32, 32, 32, 32, 26]"
    r = Prober.explain(_res(ticketFaults=1, badCUs=1, badWorkgroups=1, cusTested=255, cusVerified=254, firstBadCU=1,
                            firstBadLayer="lds", firstBadOp="ticket", firstBadSlot=0, firstBadXcc=0))
    assert r["error"] == ("AtomicResultMismatch(lds/ticket): 1 slot(s) on 1 CU(s), first on CU 0/0/0/1 slot 0; "
                          f"AtomicCoverageShort: 254/256 CUs verified, per XCD {[32] * 8}")
    ok = {"passed": True, "atomics": {"ok": True}}
    assert Prober.explain(dict(ok)) == ok
    r = _res(ok=True)  # another block's failure is not put on a clean atomics block
    r["hbm"] = {"badBits": 2, "firstBadOffset": 16}
    assert Prober.explain(r)["error"] == "HBMPatternMismatch: 2 flipped bit(s), first at offset 16"


def test_simulated_probe_reports_the_same_block():
    dev = {"uuid": "u", "index": 3, "asic": {"computeUnits": 256}}
    base = simprobe.probe(dev, {}, 0)
    assert "atomics" not in base and "atomics" not in simprobe.probe(dev, {"atomicsCheck": False}, 0)
    r = simprobe.probe(dev, {"atomicsCheck": True}, 0)
    assert r["passed"] and list(r["atomics"]) == BLOCK_KEYS and set(r) - {"atomics"} == set(base)
    b = r["atomics"]
    assert b["ok"] and b["iters"] == simprobe.SIM_ATOM_ITERS and b["layers"] == simprobe.SIM_ATOM_LAYERS == 7
    assert b["workgroups"] == simprobe.SIM_ATOM_BLOCKS_PER_CU * 256 == sum(b["wgPerXcd"])
    assert b["cusTested"] == b["cusVerified"] == 256 == sum(b["perXcd"]) and len(b["perXcd"]) == 8
    assert all(b[k] == 0 for k in BLOCK_KEYS[8:15]) and all(b[k] is None for k in BLOCK_KEYS[15:20])
    bad = simprobe.probe({**dev, "atomicsFault": 3}, {"atomicsCheck": True}, 0)
    b = bad["atomics"]
    assert not bad["passed"] and not b["ok"] and bad["hbm"]["ok"] and bad["mfma"]["ok"] and bad["cus"]["ok"]
    assert b["badCUs"] == 3 and b["cusVerified"] == 253 == sum(b["perXcd"]) and b["cusTested"] == 256
    assert (b["firstBadCU"], b["firstBadLayer"], b["firstBadOp"], b["firstBadSlot"], b["firstBadXcc"]) == (0, "lds", "add", 0, 0)
    assert Prober.explain(bad)["error"] == \
        f"AtomicResultMismatch(lds/add): {b['ldsBadSlots']} slot(s) on 3 CU(s), first on CU 0/0/0/0 slot 0"
    assert simprobe.probe({**dev, "atomicsFault": 3}, {}, 0)["passed"]  # not asked: not run
    assert simprobe.probe({**dev, "atomicsFault": 3}, {"aluCheck": True}, 0)["passed"]  # another check's overlay
    both = simprobe.probe(dev, {"aluCheck": True, "atomicsCheck": True}, 0)
    assert list(both).index("atomics") == list(both).index("alu") + 1
    # the defaults mirror the library's (native/src/probe/options.h)
    src = open(os.path.join(ROOT, "native", "src", "probe", "options.h")).read()
    ns = src[src.index("namespace atom {"):src.index("}  // namespace atom")]
    assert f"constexpr int kIters = {simprobe.SIM_ATOM_ITERS};" in ns
    assert f"constexpr int kBlocksPerCU = {simprobe.SIM_ATOM_BLOCKS_PER_CU};" in ns
    assert f"constexpr int kLayerMask = {simprobe.SIM_ATOM_LAYERS};" in ns


def test_prober_in_simulated_mode_and_gpuctl():
    p = Prober("simulated", sim_ms=0)
    dev = {"uuid": "u", "asic": {"computeUnits": 256}}
    assert p.probe_many([dev], {"atomicsCheck": True})[0]["passed"]
    r = p.probe_many([{**dev, "atomicsFault": 2}], {"atomicsCheck": True})[0]
    assert not r["passed"] and r["error"].startswith("AtomicResultMismatch(lds/add): ")
    assert p.probe_many([{**dev, "atomicsFault": 2}], {})[0]["passed"]


def test_gpuctl_describe_shows_the_verified_cus(capsys, monkeypatch):
    import types

    from gpupool.cli import gpuctl

    probe = {"passed": True, "hbmGBps": 5000.0, "mfmaTflops": 1000.0, "ms": 0.8}
    pool = {"kind": "Mi355xPool", "metadata": {"name": "p", "namespace": "default", "uid": "u1", "generation": 1},
            "status": {"devices": [{"index": 0, "uuid": "GPU-0", "health": "Healthy", "advertised": True,
                                    "probe": {**probe, "atomicsVerifiedCUs": 253}},
                                   {"index": 1, "uuid": "GPU-1", "health": "Healthy", "advertised": True, "probe": probe}]}}

    class Client:
        def get(self, res, name, ns):
            return pool

        def list(self, res, ns):
            return {"items": []}

    monkeypatch.setattr(gpuctl, "resolve", lambda c, kind: types.SimpleNamespace(namespaced=True))  # no API discovery
    assert gpuctl.cmd_describe(Client(), "default", types.SimpleNamespace(kind="mi355xpool", name="p")) == 0
    out = capsys.readouterr().out
    rows = [ln for ln in out.splitlines() if "GPU-" in ln]
    assert len(rows) == 2 and " atomics 253CU" in rows[0] and "atomics" not in rows[1], out
