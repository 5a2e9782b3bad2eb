"""spec.probe.aluCheck end to end on the fake 8x MI355X node: apiserver-sim + C++ manager + node agent
with the simulated probe."""
from __future__ import annotations

import pytest

from gpupool.kube import MI355XPOOLS
from gpupool.testing.cluster import NodeSpec

from .helpers import mi_pool, settled_events, wait_ready

pytestmark = pytest.mark.slow


def test_pool_reports_the_verified_cus_on_every_device(cluster_factory):
    k = cluster_factory(nodes=[NodeSpec("mi355x-node-0")]).client
    k.create(MI355XPOOLS, mi_pool("alu", 3, probe={"aluCheck": True}), "default")
    o = wait_ready(k, "alu", 3)
    assert o["spec"]["probe"]["aluCheck"] is True
    for d in o["status"]["devices"]:
        assert d["probe"]["passed"] and d["probe"]["aluVerifiedCUs"] == 256, d
        assert "regsVerifiedCUs" not in d["probe"] and "ldsVerifiedCUs" not in d["probe"]
    k.create(MI355XPOOLS, mi_pool("plain", 2), "default")
    o = wait_ready(k, "plain", 2)
    assert o["spec"]["probe"]["aluCheck"] is False
    assert all("aluVerifiedCUs" not in d["probe"] for d in o["status"]["devices"])


def test_a_gpu_with_a_bad_vector_alu_is_replaced(cluster_factory):
    c = cluster_factory(nodes=[NodeSpec("mi355x-node-0")])
    k = c.client
    c.set_faults("mi355x-node-0", {"devices": {"0": {"aluFault": 2}}})
    k.create(MI355XPOOLS, mi_pool("alu", 2, probe={"aluCheck": True}), "default")
    o = wait_ready(k, "alu", 2, timeout=30)
    assert 0 not in {d["index"] for d in o["status"]["devices"]}  # the pool converged on spares
    assert all(d["probe"]["aluVerifiedCUs"] == 256 for d in o["status"]["devices"])
    msgs = " ".join(e.get("message", "") for e in settled_events(k))
    assert "ALUResultMismatch(f32): 8 wave(s) on 2 CU(s), first on CU 0/0/0/0 SIMD 0 lane 0" in msgs
