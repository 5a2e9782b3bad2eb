"""The opt-in per-CU checks of the claim probe, one row each, in the order the library enqueues and
reports them. Imports nothing, so the agent's plumbing can name a check without loading the library.
"""
from __future__ import annotations

from typing import NamedTuple


class Check(NamedTuple):
    spec_key: str  # spec.probe.<key>, also the key of a probe helper's request
    option: str    # the library's option (probe.hip)
    keyword: str   # keyword of ops.probe.run
    flag: str      # flag of the mi355x-probe command line
    block: str     # the report block the check adds


CHECKS = (
    Check("ldsCheck", "ldsCheck", "lds_check", "--lds-check", "lds"),
    Check("registerCheck", "regCheck", "reg_check", "--register-check", "regs"),
    Check("aluCheck", "aluCheck", "alu_check", "--alu-check", "alu"),
    Check("atomicsCheck", "atomCheck", "atom_check", "--atomics-check", "atomics"),
)


def keywords(asked: dict) -> dict:
    """``run()`` keywords of the checks that ``asked`` (keyed by spec_key) turns on; none for the rest."""
    return {c.keyword: True for c in CHECKS if asked.get(c.spec_key)}
