"""The operator with spec.probe.mfmaLowPrecision on a real MI355X: the claim-time probe, run by the
agent's probe helper, proves the FP8 and MX block-scaled matrix cores before the GPU turns Ready."""
from __future__ import annotations

import pytest

from gpupool.kube import MI355XPOOLS
from gpupool.testing.cluster import NodeSpec

from .test_operator_gpu import pool, ready_at

pytestmark = pytest.mark.gpu
DTYPES = ["fp8", "mxfp8", "mxfp4"]


def test_pool_with_low_precision_checks_goes_ready(cluster_factory):
    c = cluster_factory(nodes=[NodeSpec("gpu-node", backend="amdsmi", probe="helper")])
    k = c.client
    k.create(MI355XPOOLS, pool("lp", 1, probe={"mfmaLowPrecision": DTYPES}), "default")
    obj = k.wait_for(MI355XPOOLS, "lp", "default", ready_at(1), timeout=60)
    d = obj["status"]["devices"][0]
    assert d["health"] == "Healthy" and d["advertised"] and d["probe"]["passed"], d
    assert d["probe"]["lowPrecisionVerified"] == DTYPES, d["probe"]
    assert d["probe"]["cusVerified"] == d["probe"]["cusExpected"]
    conds = {x["type"]: x["status"] for x in obj["status"]["conditions"]}
    assert conds["DeviceProbePassed"] == "True"
