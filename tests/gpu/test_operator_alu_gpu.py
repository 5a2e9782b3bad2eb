"""The operator with spec.probe.aluCheck on a real MI355X: the claim-time probe, run by the agent's
probe helper, runs the vector-ALU instruction program on every SIMD of every CU before the GPU turns
Ready."""
from __future__ import annotations

import pytest

from gpupool.kube import MI355XPOOLS
from gpupool.testing.cluster import NodeSpec

from .test_operator_gpu import pool, ready_at

pytestmark = pytest.mark.gpu


def test_pool_with_alu_check_goes_ready(cluster_factory):
    c = cluster_factory(nodes=[NodeSpec("gpu-node", backend="amdsmi", probe="helper")])
    k = c.client
    k.create(MI355XPOOLS, pool("alu", 1, probe={"aluCheck": True}), "default")
    obj = k.wait_for(MI355XPOOLS, "alu", "default", ready_at(1), timeout=60)
    d = obj["status"]["devices"][0]
    assert d["health"] == "Healthy" and d["advertised"] and d["probe"]["passed"], d
    assert d["probe"]["aluVerifiedCUs"] == d["probe"]["cusExpected"] > 0, d["probe"]
    assert d["probe"]["cusVerified"] == d["probe"]["cusExpected"]
    conds = {x["type"]: x["status"] for x in obj["status"]["conditions"]}
    assert conds["DeviceProbePassed"] == "True"
