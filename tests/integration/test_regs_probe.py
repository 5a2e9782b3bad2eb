"""spec.probe.registerCheck end to end on the fake 8x MI355X node: apiserver-sim + C++ manager + node
agent with the simulated probe."""
from __future__ import annotations

import pytest

from gpupool.kube import MI355XPOOLS
from gpupool.testing.cluster import NodeSpec

from .helpers import mi_pool, settled_events, wait_ready

pytestmark = pytest.mark.slow


def test_pool_reports_the_verified_cus_on_every_device(cluster_factory):
    k = cluster_factory(nodes=[NodeSpec("mi355x-node-0")]).client
    k.create(MI355XPOOLS, mi_pool("regs", 3, probe={"registerCheck": True}), "default")
    o = wait_ready(k, "regs", 3)
    assert o["spec"]["probe"]["registerCheck"] is True
    for d in o["status"]["devices"]:
        assert d["probe"]["passed"] and d["probe"]["regsVerifiedCUs"] == 256, d
        assert "ldsVerifiedCUs" not in d["probe"]
    k.create(MI355XPOOLS, mi_pool("plain", 2), "default")
    o = wait_ready(k, "plain", 2)
    assert o["spec"]["probe"]["registerCheck"] is False
    assert all("regsVerifiedCUs" not in d["probe"] for d in o["status"]["devices"])


def test_a_gpu_with_a_bad_register_file_is_replaced(cluster_factory):
    c = cluster_factory(nodes=[NodeSpec("mi355x-node-0")])
    k = c.client
    c.set_faults("mi355x-node-0", {"devices": {"0": {"regFault": 2}}})
    k.create(MI355XPOOLS, mi_pool("regs", 2, probe={"registerCheck": True}), "default")
    o = wait_ready(k, "regs", 2, timeout=30)
    assert 0 not in {d["index"] for d in o["status"]["devices"]}  # the pool converged on spares
    assert all(d["probe"]["regsVerifiedCUs"] == 256 for d in o["status"]["devices"])
    msgs = " ".join(e.get("message", "") for e in settled_events(k))
    assert ("RegisterFileMismatch: 2 flipped bit(s) on 2 CU(s), first on CU 0/0/0/0 SIMD 0 register v17 "
            "lane 0") in msgs
