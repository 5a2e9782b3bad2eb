"""spec.probe.hostLinkCheck end to end on the fake 8x MI355X node: apiserver-sim + C++ manager + node
agent with the simulated probe."""
from __future__ import annotations

import pytest

from gpupool.agent import simprobe
from gpupool.kube import MI355XPOOLS
from gpupool.testing.cluster import NodeSpec

from .helpers import mi_pool, settled_events, wait_ready

pytestmark = pytest.mark.slow


def test_pool_reports_the_link_rate_on_every_device(cluster_factory):
    k = cluster_factory(nodes=[NodeSpec("mi355x-node-0")]).client
    k.create(MI355XPOOLS, mi_pool("hl", 3, probe={"hostLinkCheck": True}), "default")
    o = wait_ready(k, "hl", 3)
    assert o["spec"]["probe"]["hostLinkCheck"] is True
    for d in o["status"]["devices"]:
        assert d["probe"]["passed"] and d["probe"]["hostLinkGBps"] == simprobe.SIM_HOSTLINK_GBPS, d
    k.create(MI355XPOOLS, mi_pool("plain", 2), "default")
    o = wait_ready(k, "plain", 2)
    assert o["spec"]["probe"]["hostLinkCheck"] is False
    assert all("hostLinkGBps" not in d["probe"] for d in o["status"]["devices"])


def test_a_gpu_behind_a_corrupting_link_is_replaced(cluster_factory):
    c = cluster_factory(nodes=[NodeSpec("mi355x-node-0")])
    k = c.client
    c.set_faults("mi355x-node-0", {"devices": {"0": {"hostLinkFail": True}}})
    k.create(MI355XPOOLS, mi_pool("hl", 2, probe={"hostLinkCheck": True}), "default")
    o = wait_ready(k, "hl", 2, timeout=30)
    assert 0 not in {d["index"] for d in o["status"]["devices"]}
    assert all(d["probe"]["hostLinkGBps"] > 0 for d in o["status"]["devices"])
    msgs = " ".join(e.get("message", "") for e in settled_events(k))
    assert "HostLinkMismatch: 1 flipped bit(s), first at offset 0" in msgs


def test_a_gpu_behind_a_slow_link_fails_the_floor_and_is_replaced(cluster_factory):
    c = cluster_factory(nodes=[NodeSpec("mi355x-node-0")])
    k = c.client
    c.set_faults("mi355x-node-0", {"devices": {"0": {"probeScale": 0.5}}})  # e.g. trained down to x8
    floor = round(simprobe.SIM_HOSTLINK_GBPS * 0.75, 1)  # between the scaled and the unscaled figure
    k.create(MI355XPOOLS, mi_pool("hl", 2, probe={"hostLinkCheck": True, "minHostLinkGBps": floor}), "default")
    o = wait_ready(k, "hl", 2, timeout=30)
    assert 0 not in {d["index"] for d in o["status"]["devices"]}
    assert all(d["probe"]["hostLinkGBps"] >= floor for d in o["status"]["devices"])
    msgs = " ".join(e.get("message", "") for e in settled_events(k))
    assert "PerformanceBelowFloor" in msgs
    assert f"host link {simprobe.SIM_HOSTLINK_GBPS * 0.5:.1f} GB/s < floor {floor:.1f}" in msgs
