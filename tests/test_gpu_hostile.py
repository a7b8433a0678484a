"""GPU: the general-path fuzz's hostile groups (simplex, duplex, CODEC) spliced into the layout tests' backgrounds — at the first and last
group, inside the first 64 families (the build-choice sample), at forced chunk boundaries — through both entries against the oracle, with
tensors in HBM (tests/layout_runs.py).  No background group may be deferred, and a stated share of the hostile groups must be decided on
the device.  FGX_FUZZ_ROUNDS scales the seeds, as in tests/test_general_path_fuzz.py."""
import os

import pytest

from isolated import run_isolated

pytestmark = pytest.mark.gpu

ROUNDS = int(os.environ.get("FGX_FUZZ_ROUNDS", "12"))
# the share of hostile groups the device must decide: CODEC and duplex molecules of the fuzz are mostly outside the canonical form's scope
SHARE = {"codec": 0.05, "duplex": 0.1}
HEADS = {"seg4": 20000, "packed": 20000, "pair": 20000, "deep": 1500, "trim": 5000, "wave2": 5000, "duplex": 5000, "codec": 5000}


@pytest.mark.parametrize("head", list(HEADS))
def test_hostile_groups_on_the_gpu(head):
    env = {"FGX_SPLIT": "0"} if head == "wave2" else {}
    seeds = [8000 + 100 * list(HEADS).index(head) + s for s in range(max(2, ROUNDS // 3))]
    run_isolated("layout_runs", "check_hostile", head, HEADS[head], seeds, 16, "device", None, SHARE.get(head, 0.25), env=env, timeout=900)


def test_hostile_groups_at_the_chunk_boundaries_on_the_gpu():
    """FGX_SPLIT_CHUNKS=4 over 20 000 depth-8 families: hostile groups on both sides of every chunk boundary (placed by the product's chunk
    geometry, asserted in layout_runs.check)."""
    run_isolated("layout_runs", "check_hostile", "packed", 20000, [8900, 8901], 16, "device", 4, env={"FGX_SPLIT_CHUNKS": "4"}, timeout=900)


def test_hostile_records_inside_deep_families_on_the_gpu():
    run_isolated("layout_runs", "check_hostile_deep", 1500, [8950, 8951], "device", timeout=900)
