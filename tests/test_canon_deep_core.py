"""canon_core.h at 512 records (fgx_canon_duplex_deep_host: the scalar form k_canon_duplex_deep is compared with), through the oracle alone.  The claim is
tests/test_canon_core.py's: for every in-scope molecule M the reference's result for the canonical molecule C(M), plus the statistics the canonicalisation counted
itself, IS the reference's result for M, byte for byte and counter for counter — here for molecules of 65 .. 512 records.  For molecules of up to 128 records the
hook's bytes are fgx_canon_duplex_host's, which keeps refusing above 128."""
import random

import numpy as np
import pytest

import bamutil
import deep_indel_cases as D
import fgx_opts
import test_canon_core as tc
from fgumi_amd._lib import lib

N_SEEDS = 64


def seeded_molecule(seed):
    """A deep molecule over test_canon_core's 13 CIGAR pairs (so the 16-group bound cannot bite): a majority pair, one template in ten of another pair."""
    rng = random.Random(4000 + seed)
    templates = rng.choice([33, 34, 40, 48, 64, 65, 80, 100]) if seed % 8 else rng.choice([200, 255, 256])
    n_a = rng.randint(templates // 4, templates - templates // 4)
    minority = {t: rng.randrange(len(tc.C1)) for t in range(templates) if rng.random() < 0.1}
    if templates == 256 and not minority:
        minority = {3: D.INS}
    return D.molecule(seed, n_a, templates - n_a, major=rng.randrange(len(tc.C1)), minority=minority, g=seed, insert=rng.choice([110, 140, 180, 260]),
                      start=rng.randint(10, 3000), err=0.01)


def check_molecule(o, recs):
    """test_canon_core.check_molecule on the 512-record hook.  Returns the reads the filter dropped, or None when the molecule is out of scope."""
    c = D.canonical(o, recs)
    if c["status"] != 0:
        return None
    canon = [r for r in c["recs"] if r]
    want = tc.oracle(o, [recs])
    got = tc.oracle(o, [canon]) if canon else dict(data=b"", count=0, stats=np.zeros(28, dtype=np.uint64))
    assert got["data"] == want["data"], "records differ"
    st = got["stats"].copy()
    delta = c["delta"]
    st[0] += delta[0]; st[2] += delta[0]; st[tc.MINORITY] += delta[0]
    assert not got["stats"][24:28].any()
    st[24:28] += np.array(delta[1:5], dtype=np.uint64)
    assert np.array_equal(st, want["stats"]), (st.tolist(), want["stats"].tolist(), delta)
    for r in canon:
        p = bamutil.parse(r)
        assert p["n_cigar"] == (1 if p["seq"] else 0) and "MC" not in p["tags"]
    return int(delta[0])


def test_canonical_deep_molecules_give_the_original_result():
    """>= 60 seeded molecules of 66 .. 512 records under the default options: at least 80 % in scope, and the filter drops reads."""
    o = fgx_opts.defaults(kind=1)
    sizes, in_scope, dropped = [], 0, 0
    for seed in range(N_SEEDS):
        recs = seeded_molecule(seed)
        assert 64 < len(recs) <= 512
        sizes.append(len(recs))
        d = check_molecule(o, recs)
        if d is not None:
            in_scope += 1
            dropped += d
    print(f"{N_SEEDS} molecules of {min(sizes)} .. {max(sizes)} records: {in_scope} in scope, {dropped} reads dropped")
    assert N_SEEDS >= 60 and max(sizes) > 500 and in_scope >= 0.8 * N_SEEDS and dropped > 0, (in_scope, dropped)


@pytest.mark.parametrize("i", range(len(D.OPTION_SETS)))
def test_the_claim_holds_under_the_option_sets(i):
    for seed in (1, 2, 3, 9):
        case = D.with_option_set(D.Case(seeded_molecule(seed)), i)
        check_molecule(D.options_of(case), case.recs)


@pytest.mark.parametrize("name", [n for n in D.CASES if n not in ("510_records", "512_records", "514_records")])
def test_the_claim_holds_for_the_shapes(name):
    """The hand-made shapes of tests/deep_indel_cases.py: in scope or not as the case says, and the claim where it is."""
    case = D.CASES[name]()
    d = check_molecule(D.options_of(case), case.recs)
    assert (d is not None) == case.in_scope
    if case.in_scope and case.dropped >= 0:
        assert d == case.dropped


def test_identity_with_the_hook_at_128_records():
    """Up to 128 records both hooks give the same status, delta, lengths and bytes; above, fgx_canon_duplex_host refuses and the new hook does not; above 512 both."""
    o = fgx_opts.defaults(kind=1)
    rng = random.Random(77)
    compared = 0
    for g in range(60):
        recs = tc.duplex_indel_molecule(rng, g)
        if recs:
            a, b = D.canonical(o, recs, "fgx_canon_duplex_host"), D.canonical(o, recs)
            assert a == b
            compared += a["status"] == 0
    assert compared > 30
    for name in ("66_records", "128_records", "two_equal_groups_smaller_first", "16_groups", "17_groups", "first_record_dropped_other_cb"):
        case = D.CASES[name]()
        oc = D.options_of(case)
        a, b = D.canonical(oc, case.recs, "fgx_canon_duplex_host"), D.canonical(oc, case.recs)
        assert a["status"] == b["status"] == (0 if case.in_scope else 1)
        if case.in_scope:
            assert a == b
    big = D.CASES["130_records"]()
    assert D.canonical(o, big.recs, "fgx_canon_duplex_host")["status"] == 1 and D.canonical(o, big.recs)["status"] == 0
    assert D.canonical(o, D.CASES["514_records"]().recs)["status"] == 1


def test_bad_arguments():
    assert lib.fgx_canon_duplex_deep_host(None, None, None, None, 0, None, None, None) == 2
