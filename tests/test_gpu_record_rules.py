"""Edge records at the call sites of the record rules (record_core.h) on the GPU: per head of the launch chain one small batch per edge (a few hundred records
each) through both entries against the oracle, and the route each batch took against the recorded table.  Cases, rules and checks: tests/record_rule_cases.py."""
import pytest

from isolated import run_isolated
from record_rule_cases import HEADS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("head", list(HEADS))
def test_record_rules_on_the_device(head):
    run_isolated("record_rule_cases", "check", head, "device", env=HEADS[head][2])
