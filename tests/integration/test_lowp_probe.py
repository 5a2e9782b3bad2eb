"""spec.probe.mfmaLowPrecision end to end on the fake 8x MI355X node: apiserver-sim + C++ manager +
node agent with the simulated probe."""
from __future__ import annotations

import pytest

from gpupool.kube import MI355XPOOLS
from gpupool.testing.cluster import NodeSpec

from .helpers import mi_pool, settled_events, wait_ready

pytestmark = pytest.mark.slow


def test_pool_lists_the_verified_dtypes_on_every_device(cluster_factory):
    k = cluster_factory(nodes=[NodeSpec("mi355x-node-0")]).client
    k.create(MI355XPOOLS, mi_pool("lp", 3, probe={"mfmaLowPrecision": ["fp8", "mxfp4"]}), "default")
    o = wait_ready(k, "lp", 3)
    assert o["spec"]["probe"]["mfmaLowPrecision"] == ["fp8", "mxfp4"]
    for d in o["status"]["devices"]:
        assert d["probe"]["passed"] and d["probe"]["lowPrecisionVerified"] == ["fp8", "mxfp4"], d
    k.create(MI355XPOOLS, mi_pool("plain", 2), "default")
    o = wait_ready(k, "plain", 2)
    assert o["spec"]["probe"]["mfmaLowPrecision"] == []
    assert all("lowPrecisionVerified" not in d["probe"] for d in o["status"]["devices"])


def test_a_gpu_that_fails_one_dtype_is_replaced(cluster_factory):
    c = cluster_factory(nodes=[NodeSpec("mi355x-node-0")])
    k = c.client
    c.set_faults("mi355x-node-0", {"devices": {"0": {"lowpFault": "mxfp4"}}})
    k.create(MI355XPOOLS, mi_pool("lp", 2, probe={"mfmaLowPrecision": ["fp8", "mxfp4"]}), "default")
    o = wait_ready(k, "lp", 2, timeout=30)
    assert 0 not in {d["index"] for d in o["status"]["devices"]}
    assert all(d["probe"]["lowPrecisionVerified"] == ["fp8", "mxfp4"] for d in o["status"]["devices"])
    msgs = " ".join(e.get("message", "") for e in settled_events(k))
    assert "MFMAResultMismatch(mxfp4): 0 element / 2 ABFT mismatch(es)" in msgs
