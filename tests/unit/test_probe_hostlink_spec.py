"""spec.probe.hostLinkCheck / hostLinkBytes / minHostLinkGBps through the public layers, on the CPU:
the schema and the CRD's admission (defaults, bounds, the CEL rule), the manager's API layer (C++),
the bindings' option encoding, the agent's probe plumbing and wording, and the simulated probe."""
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
from gpupool.ops import probe as hp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
POOLS = ("compute.my.domain", "mi355xpools")
BLOCK_KEYS = {"ok", "bytes", "patterns", "seed", "badBits", "firstBadOffset", "hostSamples",
              "hostSampleMismatches", "writeGBps", "readGBps", "GBps", "ms", "allocMs"}


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


def test_schema_declares_the_fields_and_the_status():
    crd = yaml.safe_load(open(os.path.join(ROOT, "config", "crd", "compute.my.domain_mi355xpools.yaml")))
    root = crd["spec"]["versions"][0]["schema"]["openAPIV3Schema"]["properties"]
    pr = root["spec"]["properties"]["probe"]["properties"]
    assert pr["hostLinkCheck"]["type"] == "boolean" and pr["hostLinkCheck"]["default"] is False
    b = pr["hostLinkBytes"]
    assert (b["minimum"], b["maximum"], b["default"]) == (1 << 20, 1 << 30, schema.DEFAULT_HOST_LINK_BYTES)
    assert b["default"] & (b["default"] - 1) == 0  # a power of two
    assert pr["minHostLinkGBps"]["minimum"] == 0 and pr["minHostLinkGBps"]["default"] == 0
    assert any("minHostLinkGBps" in r["rule"] for r in root["spec"]["x-kubernetes-validations"])
    st = root["status"]["properties"]["devices"]["items"]["properties"]["probe"]["properties"]
    assert st["hostLinkGBps"]["type"] == "number"


def test_crd_defaults_and_accepts(store):
    p = _create(store, "d", {})["spec"]["probe"]
    assert p["hostLinkCheck"] is False and p["hostLinkBytes"] == schema.DEFAULT_HOST_LINK_BYTES
    assert p["minHostLinkGBps"] == 0
    p = _create(store, "on", {"hostLinkCheck": True, "hostLinkBytes": 1 << 20, "minHostLinkGBps": 40})["spec"]["probe"]
    assert p["hostLinkCheck"] is True and p["hostLinkBytes"] == 1 << 20 and p["minHostLinkGBps"] == 40
    _create(store, "max", {"hostLinkCheck": True, "hostLinkBytes": 1 << 30})
    _create(store, "zero", {"hostLinkCheck": False, "minHostLinkGBps": 0})


@pytest.mark.parametrize("probe,needle", [
    ({"hostLinkCheck": True, "hostLinkBytes": (1 << 20) - 1}, "hostLinkBytes"),
    ({"hostLinkCheck": True, "hostLinkBytes": (1 << 30) + 1}, "hostLinkBytes"),
    ({"hostLinkCheck": True, "minHostLinkGBps": -1}, "minHostLinkGBps"),
    ({"hostLinkCheck": "yes"}, "hostLinkCheck"),
    ({"minHostLinkGBps": 40}, "needs probe.hostLinkCheck"),
    ({"hostLinkCheck": False, "minHostLinkGBps": 0.5}, "needs probe.hostLinkCheck"),
])
def test_crd_refuses(store, probe, needle):
    with pytest.raises(ApiError) as e:
        _create(store, "bad", probe)
    assert needle in str(e.value.message if hasattr(e.value, "message") else e.value)


def test_manager_api_layer(native_built):
    """native/tests/test_hostlink_spec.cc: parse, probe_json / policy_json, InvalidSpec, hostLinkGBps."""
    r = subprocess.run([os.path.join(native_built, "gpupool_tests"), "hostlink_"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "3 passed, 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def test_run_opts_default_encoding_is_unchanged():
    base = hp._run_opts(1 << 30, True, 4096, 2, 1, 256, ())
    assert base == (b'{"hbmBytes": 1073741824, "mfma": true, "gemmN": 4096, "patterns": 2, "gemmReps": 1, '
                    b'"gemmTile": 256}')
    assert hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 0) == base
    on = json.loads(hp._run_opts(1 << 30, True, 4096, 2, 1, 256, (), (), 4 << 20))
    assert on == {**json.loads(base), "hostLinkBytes": 4 << 20}
    both = json.loads(hp._run_opts(1 << 30, True, 2048, 2, 1, 256, (("overlap", 1),), ("fp8",), 1 << 20))
    assert both["hostLinkBytes"] == 1 << 20 and both["mfmaLowPrecision"] == 1 and both["overlap"] == 1


class _Helpers:
    """Stands in for the helper pool: records the args of each call."""

    def __init__(self, res):
        self.calls, self.res = [], res

    def get(self, uuid, dev):
        return self

    def call(self, op, args, timeout):
        self.calls.append((op, args))
        return dict(self.res)


def test_helper_args_carry_the_size_only_when_asked_for():
    p = Prober("simulated", sim_ms=0)
    p.mode = "helper"
    p.helpers = h = _Helpers({"passed": True})
    dev = {"uuid": "u", "hipUUID": "GPU-0", "index": 0}
    p._one(dev, {})
    p._one(dev, {"hostLinkBytes": 8 << 20})  # the CRD's default is there, the check is not asked for
    p._one(dev, {"hostLinkCheck": True, "hostLinkBytes": 8 << 20})
    p._one(dev, {"hostLinkCheck": True})
    p._one(dev, {"hostLinkCheck": True, "hostLinkBytes": 8 << 20, "minHostLinkGBps": 30})
    a = [args for _, args in h.calls]
    assert "hostLinkBytes" not in a[0] and "hostLinkBytes" not in a[1]
    assert set(a[0]) == {"hipUUID", "hbmBytes", "mfma", "gemmN", "overlap", "hooks"}
    assert a[2]["hostLinkBytes"] == 8 << 20 and a[2]["overlap"] == 1 and a[2]["gemmN"] == p.overlap_gemm_n
    assert a[3]["hostLinkBytes"] == schema.DEFAULT_HOST_LINK_BYTES
    assert a[4]["overlap"] == 0 and a[4]["gemmN"] == p.gemm_n  # a floor: serial probe, clean numbers
    # a floor without the check measures nothing and must not make the probe serial
    p._one(dev, {"minHostLinkGBps": 30})
    assert h.calls[-1][1]["overlap"] == 1


def test_helper_op_passes_the_size_to_the_binding():
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
    assert k.hp.kw["host_link_bytes"] == 0
    k.call("probe", {**base, "hostLinkBytes": 2 << 20})
    assert k.hp.kw["host_link_bytes"] == 2 << 20


def _res(**link):
    return {"passed": False, "hbm": {"badBits": 0}, "mfma": {"elementMismatches": 0, "abftMismatches": 0},
            "cus": {"expected": 256, "mfmaVerified": 256, "badWaves": 0, "ok": True},
            "hostLink": {"ok": False, "badBits": 0, "firstBadOffset": None, "hostSamples": 1026,
                         "hostSampleMismatches": 0, **link}}


def test_explain_wording():
    r = Prober.explain(_res(badBits=3, firstBadOffset=4096))
    assert r["error"] == "HostLinkMismatch: 3 flipped bit(s), first at offset 4096"
    r = Prober.explain(_res(hostSampleMismatches=2))
    assert r["error"] == "HostLinkMismatch: 2 of 1026 host samples differ"
    r = Prober.explain(_res(badBits=1, firstBadOffset=0, hostSampleMismatches=1))
    assert r["error"] == "HostLinkMismatch: 1 flipped bit(s), first at offset 0, 1 of 1026 host samples differ"
    ok = {"passed": True, "hostLink": {"ok": True, "badBits": 0}}
    assert Prober.explain(dict(ok)) == ok


def _measured(gbps):
    return {"passed": True, "hbm": {"GBps": 4900.0}, "mfma": {"tflops": 1200.0, "enabled": True},
            "hostLink": {"ok": True, "GBps": gbps}}


def test_apply_floors_wording_and_scale():
    r = Prober.apply_floors(_measured(31.26), {}, {"hostLinkCheck": True, "minHostLinkGBps": 45})
    assert not r["passed"] and r["error"] == "PerformanceBelowFloor: host link 31.3 GB/s < floor 45.0"
    assert Prober.apply_floors(_measured(52.0), {}, {"hostLinkCheck": True, "minHostLinkGBps": 45})["passed"]
    assert Prober.apply_floors(_measured(52.0), {}, {"hostLinkCheck": True, "minHostLinkGBps": 0})["passed"]
    r = Prober.apply_floors(_measured(52.0), {"faults": {"probeScale": 0.5}},
                            {"hostLinkCheck": True, "minHostLinkGBps": 45, "minHbmGBps": 3000})
    assert r["hostLink"]["GBps"] == 26.0
    assert r["error"] == "PerformanceBelowFloor: HBM 2450 GB/s < floor 3000; host link 26.0 GB/s < floor 45.0"
    plain = {"passed": True, "hbm": {"GBps": 4900.0}, "mfma": {"tflops": 1200.0}}
    assert Prober.apply_floors(dict(plain), {}, {"minHostLinkGBps": 45})["passed"]  # no block: nothing measured


def test_simulated_probe_reports_the_same_block():
    dev = {"uuid": "u", "index": 3, "asic": {"computeUnits": 256}}
    base = simprobe.probe(dev, {}, 0)
    assert "hostLink" not in base
    assert "hostLink" not in simprobe.probe(dev, {"hostLinkBytes": 8 << 20}, 0)  # size alone asks for nothing
    r = simprobe.probe(dev, {"hostLinkCheck": True, "hostLinkBytes": 8 << 20}, 0)
    assert r["passed"] and set(r["hostLink"]) == BLOCK_KEYS and set(r) - {"hostLink"} == set(base)
    h = r["hostLink"]
    assert h["ok"] and h["bytes"] == 8 << 20 and h["seed"] == 0x4C4B0003 and h["firstBadOffset"] is None
    assert h["GBps"] == simprobe.SIM_HOSTLINK_GBPS == min(h["writeGBps"], h["readGBps"]) <= 63
    assert simprobe.probe(dev, {"hostLinkCheck": True}, 0)["hostLink"]["bytes"] == schema.DEFAULT_HOST_LINK_BYTES
    bad = simprobe.probe({**dev, "hostLinkFail": True}, {"hostLinkCheck": True}, 0)
    assert not bad["passed"] and not bad["hostLink"]["ok"]
    assert bad["hostLink"]["badBits"] == 1 and bad["hostLink"]["firstBadOffset"] == 0
    assert Prober.explain(bad)["error"] == "HostLinkMismatch: 1 flipped bit(s), first at offset 0"
    assert simprobe.probe({**dev, "hostLinkFail": True}, {}, 0)["passed"]  # not asked: not run


def test_prober_in_simulated_mode_with_scale_and_floor():
    p = Prober("simulated", sim_ms=0)
    dev = {"uuid": "u", "asic": {"computeUnits": 256}}
    opts = {"hostLinkCheck": True, "minHostLinkGBps": simprobe.SIM_HOSTLINK_GBPS * 0.75}
    assert p.probe_many([dev], opts)[0]["passed"]
    r = p.probe_many([{**dev, "probeScale": 0.5}], opts)[0]
    assert not r["passed"] and r["error"].startswith("PerformanceBelowFloor: host link ")
    assert r["hostLink"]["GBps"] == simprobe.SIM_HOSTLINK_GBPS * 0.5
    r = p.probe_many([{**dev, "hostLinkFail": True}], opts)[0]
    assert not r["passed"] and r["error"].startswith("HostLinkMismatch: 1 flipped bit(s)")
