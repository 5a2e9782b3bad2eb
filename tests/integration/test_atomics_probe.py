"""spec.probe.atomicsCheck end to end on the fake 8x MI355X node: apiserver-sim + C++ manager + node agent
with the simulated probe."""
from __future__ import annotations

import pytest

from gpupool.kube import MI355XPOOLS
from gpupool.testing.cluster import NodeSpec

from .helpers import mi_pool, settled_events, wait_ready

pytestmark = pytest.mark.slow


def test_pool_reports_the_verified_cus_on_every_device(cluster_factory):
    k = cluster_factory(nodes=[NodeSpec("mi355x-node-0")]).client
    k.create(MI355XPOOLS, mi_pool("atomics", 3, probe={"atomicsCheck": True}), "default")
    o = wait_ready(k, "atomics", 3)
    assert o["spec"]["probe"]["atomicsCheck"] is True
    for d in o["status"]["devices"]:
        assert d["probe"]["passed"] and d["probe"]["atomicsVerifiedCUs"] == 256, d
        assert "aluVerifiedCUs" not in d["probe"] and "ldsVerifiedCUs" not in d["probe"]


def test_a_pool_without_the_option_sends_and_reports_nothing(cluster_factory):
    k = cluster_factory(nodes=[NodeSpec("mi355x-node-0")]).client
    k.create(MI355XPOOLS, mi_pool("plain", 2), "default")
    o = wait_ready(k, "plain", 2)
    assert o["spec"]["probe"]["atomicsCheck"] is False
    assert all("atomicsVerifiedCUs" not in d["probe"] for d in o["status"]["devices"])
    # what the manager sends with a claim: the option is absent, not false, so no "atomCheck" reaches the library
    from gpupool.agent.prober import Prober

    class Helpers:
        calls = []

        def get(self, uuid, dev):
            return self

        def call(self, op, args, timeout):
            self.calls.append(args)
            return {"passed": True}

    p = Prober("simulated", sim_ms=0)
    p.mode, p.helpers = "helper", Helpers()
    p._one({"uuid": "u", "hipUUID": "GPU-0", "index": 0}, dict(o["spec"]["probe"]))
    assert "atomicsCheck" not in Helpers.calls[0]


def test_a_gpu_with_a_bad_atomic_unit_is_replaced(cluster_factory):
    c = cluster_factory(nodes=[NodeSpec("mi355x-node-0")])
    k = c.client
    c.set_faults("mi355x-node-0", {"devices": {"0": {"atomicsFault": 3}}})
    k.create(MI355XPOOLS, mi_pool("atomics", 2, probe={"atomicsCheck": True}), "default")
    o = wait_ready(k, "atomics", 2, timeout=30)
    assert 0 not in {d["index"] for d in o["status"]["devices"]}  # the pool converged on spares
    assert all(d["probe"]["atomicsVerifiedCUs"] == 256 for d in o["status"]["devices"])
    msgs = " ".join(e.get("message", "") for e in settled_events(k))
    assert "AtomicResultMismatch(lds/add): 3 slot(s) on 3 CU(s), first on CU 0/0/0/0 slot 0" in msgs
