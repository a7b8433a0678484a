"""Edge records at the call sites of the record rules (record_core.h) under the wave-level host emulator: per head of the launch chain one small batch per
edge through both entries against the oracle, and the route each batch took against the table recorded from the commit before the parsers were rewritten
(tests/golden/record_rule_routes.json).  Cases, rules and checks: tests/record_rule_cases.py."""
import pytest

from isolated import run_isolated
from record_rule_cases import HEADS
from test_wavemu import env


@pytest.mark.parametrize("head", list(HEADS))
def test_record_rules_under_the_emulator(head):
    run_isolated("record_rule_cases", "check", head, "host", env=env(**HEADS[head][2]), timeout=1500)
