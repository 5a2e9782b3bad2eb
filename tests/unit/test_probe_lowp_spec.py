"""spec.probe.mfmaLowPrecision through the public layers, on the CPU: the schema and the CRD's
admission (enum, uniqueness, the CEL rule), the manager's API layer (C++), the agent's probe
plumbing and wording, and the simulated probe."""
from __future__ import annotations

import glob
import os
import subprocess

import pytest
import yaml

from gpupool.agent import simprobe
from gpupool.agent.prober import Prober
from gpupool.api import schema
from gpupool.apiserver_sim.store import ApiError, Store

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
POOLS = ("compute.my.domain", "mi355xpools")


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
    f = root["spec"]["properties"]["probe"]["properties"]["mfmaLowPrecision"]
    assert f["default"] == [] and f["items"]["enum"] == ["fp8", "mxfp8", "mxfp4"]
    assert f["x-kubernetes-list-type"] == "set"
    assert any("mfmaLowPrecision" in r["rule"] for r in root["spec"]["x-kubernetes-validations"])
    st = root["status"]["properties"]["devices"]["items"]["properties"]["probe"]["properties"]
    assert st["lowPrecisionVerified"]["items"]["enum"] == list(schema.LOW_PRECISION_DTYPES)
    from gpupool.ops import lowp
    assert schema.LOW_PRECISION_DTYPES == lowp.DTYPES


def test_crd_defaults_and_accepts(store):
    assert _create(store, "d", {})["spec"]["probe"]["mfmaLowPrecision"] == []
    o = _create(store, "ok", {"mfmaLowPrecision": ["fp8", "mxfp4"]})
    assert o["spec"]["probe"]["mfmaLowPrecision"] == ["fp8", "mxfp4"]
    _create(store, "off", {"mfma": False, "mfmaLowPrecision": []})


@pytest.mark.parametrize("probe,needle", [
    ({"mfmaLowPrecision": ["fp6"]}, "mfmaLowPrecision"),
    ({"mfmaLowPrecision": ["fp8", "fp8"]}, "Duplicate"),
    ({"mfmaLowPrecision": ["fp8", "mxfp8", "mxfp4", "fp8"]}, "mfmaLowPrecision"),
    ({"mfma": False, "mfmaLowPrecision": ["mxfp8"]}, "needs probe.mfma"),
])
def test_crd_refuses(store, probe, needle):
    with pytest.raises(ApiError) as e:
        _create(store, "bad", probe)
    assert needle in str(e.value.message if hasattr(e.value, "message") else e.value)


def test_manager_api_layer(native_built):
    """native/tests/test_lowp_spec.cc: parse, probe_json, InvalidSpec, lowPrecisionVerified."""
    r = subprocess.run([os.path.join(native_built, "gpupool_tests"), "lowp_"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "3 passed, 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def _res(**lowp):
    return {"passed": False, "hbm": {"badBits": 0}, "mfma": {"elementMismatches": 0, "abftMismatches": 0},
            "cus": {"expected": 256, "mfmaVerified": 256, "badWaves": 0, "ok": True}, "lowp": lowp}


def test_explain_names_the_dtype():
    ok = {"ok": True, "elementMismatches": 0, "abftMismatches": 0, "cusVerified": 256, "badWaves": 0}
    r = Prober.explain(_res(fp8=ok, mxfp4={**ok, "ok": False, "abftMismatches": 2}))
    assert r["error"] == "MFMAResultMismatch(mxfp4): 0 element / 2 ABFT mismatch(es)"
    r = Prober.explain(_res(fp8={**ok, "ok": False, "cusVerified": 248, "badWaves": 64}))
    assert r["error"].startswith("CUCensusFailed(fp8): 248/256 ")
    r = Prober.explain(_res(mxfp8={**ok, "ok": False, "elementMismatches": 3},
                            mxfp4={**ok, "ok": False, "cusVerified": 224, "badWaves": 8}))
    assert "MFMAResultMismatch(mxfp8): 3 element / 0 ABFT" in r["error"] and "CUCensusFailed(mxfp4): 224/256" in r["error"]
    passed = {"passed": True, "lowp": {"fp8": ok}}
    assert Prober.explain(dict(passed)) == passed


def test_simulated_probe_reports_the_same_block():
    dev = {"uuid": "u", "asic": {"computeUnits": 256}}
    base = simprobe.probe(dev, {}, 0)
    assert "lowp" not in base
    r = simprobe.probe(dev, {"mfmaLowPrecision": ["fp8", "mxfp4"]}, 0)
    assert r["passed"] and list(r["lowp"]) == ["fp8", "mxfp4"]
    assert set(r["lowp"]["fp8"]) == {"ok", "n", "elementMismatches", "abftMismatches", "tflops", "ms",
                                     "cusVerified", "badWaves"}
    assert set(r) - {"lowp"} == set(base)
    r = simprobe.probe({**dev, "lowpFault": "mxfp4"}, {"mfmaLowPrecision": ["fp8", "mxfp4"]}, 0)
    assert not r["passed"] and r["lowp"]["fp8"]["ok"] and not r["lowp"]["mxfp4"]["ok"]
    assert "MFMAResultMismatch(mxfp4)" in Prober.explain(r)["error"]
    r = simprobe.probe({**dev, "lowpFault": "mxfp4"}, {"mfmaLowPrecision": ["fp8"]}, 0)  # not asked: not run
    assert r["passed"]


def test_prober_passes_the_list_in_simulated_mode():
    p = Prober("simulated", sim_ms=0)
    dev = {"uuid": "u", "asic": {"computeUnits": 256}}
    r = p.probe_many([dev], {"mfmaLowPrecision": ["mxfp8"]})[0]
    assert r["passed"] and list(r["lowp"]) == ["mxfp8"]
    r = p.probe_many([{**dev, "lowpFault": "mxfp8"}], {"mfmaLowPrecision": ["mxfp8"]})[0]
    assert not r["passed"] and r["error"].startswith("MFMAResultMismatch(mxfp8)")
