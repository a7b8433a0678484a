"""Every build of the per-field record writers (fgumi_amd/csrc/record_writers.inc: k_emit_duplex<0>, <1>, <0, 1>, k_emit_codec), executed on the CPU in
64-lane lock-step (tests/wavemu): bytes, count and counters of fgx_process_batch_device against the oracle, nothing deferred.  The per-field kernels are
launched only when k_count_slow counted a record the fast writers (k_emit_duplex_fast / k_emit_codec_fast) refuse — a long name or tag, or a duplex
record of more than 256 positions — so every batch here is built to hold such records, and says so from the expected output.  The same batches run on
the GPU in tests/test_gpu_duplex.py, tests/test_gpu_codec.py, tests/test_gpu_duplex_methylation_device.py and tests/test_gpu_strand_cap.py."""
import pytest

import bamutil
from isolated import run_isolated
from test_wavemu import env

DUPLEX_SIM = dict(family_size=6, duplex=1)
CODEC_SIM = dict(family_size=3, read_length=150, insert_mean=200, insert_sd=30, codec=1)
LONG_DUPLEX_SIM = dict(family_size=3, read_length=300, insert_mean=350, insert_sd=30, duplex=1)
CODEC_MASKS = dict(overlapping_consensus=0, produce_per_base_tags=1, codec_has_outer_bases_qual=1, codec_outer_bases_qual=5, codec_outer_bases_length=90,
                   codec_has_single_strand_qual=1, codec_single_strand_qual=4)


def writer_counts(data):
    """(records the fast writers take, records they leave to the per-field writers) by name length: l_read_name <= 64 or not (small_tags)."""
    from fgumi_amd import split_records
    names = [r[8] for r in split_records(data)]
    return sum(n <= 64 for n in names), sum(n > 64 for n in names)


def r1_orientations(g):
    """The strands of the first-of-pair records of a batch: {False, True} when both orientations of R1 occur."""
    seen = set()
    for r in range(g.n_rec):
        off, ln = int(g.rec_off[r]), int(g.rec_len[r])
        flag = bamutil.parse(bytes(g.blob[off:off + ln]))["flag"]
        if flag & 0x40:
            seen.add(bool(flag & 0x10))
    return seen


def check_both_writers_own_records(kind, n):
    """A 60-character prefix: the name crosses 64 bytes between two- and three-digit MIs, so one batch holds records of the fast writer and of the
    per-field writer."""
    from fgumi_amd import simulate_grouped_reads
    from test_wavemu_strand_cap import device_entry
    g = simulate_grouped_reads(n, **(DUPLEX_SIM if kind == 1 else CODEC_SIM))
    opts = dict(min_reads=1) if kind == 1 else dict(overlapping_consensus=0)
    _, want = device_entry(kind, g, read_name_prefix=b"p" * 60, **opts)
    fast, slow = writer_counts(want["data"])
    print(f"kind {kind}: {fast} records for the fast writer, {slow} for the per-field writer")
    assert fast > 0 and slow > 0, (fast, slow)


def check_duplex_refused_for_length(n):
    """Reads of 300 bases: duplex records above 128 * DUP_SLOTS positions, which k_emit_duplex_fast refuses whatever their names."""
    from fgumi_amd import simulate_grouped_reads
    from test_wavemu_strand_cap import device_entry
    recs, _ = device_entry(1, simulate_grouped_reads(n, **LONG_DUPLEX_SIM), min_reads=1)
    assert sum(len(r["seq"]) > 256 for r in recs) > n, [len(r["seq"]) for r in recs[:8]]


def check_methylation_build():
    """k_emit_duplex<1>: the smallest methylation batch of tests/test_wavemu_duplex_methylation.py under a 70-character prefix."""
    import test_wavemu_duplex_methylation as m
    m.check_device_entry(1, (1, 1, 0), 72, 300, read_name_prefix=b"m" * 70)


def capped_molecule():
    """The crafted molecule of test_wavemu_strand_cap.check_dropped_read_counts_in_the_recount: the read the cap drops is the only one that disagrees."""
    import test_wavemu_strand_cap as sc
    s = sc.names_by_rank(3)
    return sc.duplex_molecule([(s[0], sc.BASE, 37), (s[1], sc.BASE, 37), (s[2], sc.with_base("C", col=7), 37)])


def cap_changes_the_recount(capped, uncapped):
    """From the oracle's records: the cap bit, and the error recount shows it — a record whose cE is not the cap-off run's."""
    assert len(capped) == len(uncapped) > 0
    assert any(a["tags"]["cE"][1] != b["tags"]["cE"][1] for a, b in zip(capped, uncapped)), [r["tags"]["cE"] for r in capped + uncapped]


def check_cap_build():
    """k_emit_duplex<0, 1> with a record whose recount reads col_obs_all, under a 70-character prefix."""
    import test_wavemu_strand_cap as sc
    g = capped_molecule()
    prefix = b"k" * 70
    capped, want = sc.device_entry(1, g, duplex_max_reads_per_strand=2, read_name_prefix=prefix)
    uncapped, _ = sc.oracle_only(1, g, read_name_prefix=prefix)
    assert writer_counts(want["data"]) == (0, len(capped))
    cap_changes_the_recount(capped, uncapped)


def check_codec_orientations_and_masks(n):
    """k_emit_codec with per-base tags and both quality masks on, on molecules of both orientations of R1."""
    from fgumi_amd import simulate_grouped_reads
    from test_wavemu_strand_cap import device_entry
    g = simulate_grouped_reads(n, **CODEC_SIM)
    assert r1_orientations(g) == {False, True}
    recs, want = device_entry(2, g, read_name_prefix=b"c" * 70, **CODEC_MASKS)
    assert writer_counts(want["data"]) == (0, len(recs)) and len(recs) > n // 2
    # both masks are live in the expected output: the outer 90 bases reach into the two-strand stretch and show the outer quality there, the
    # single-strand stretches ('n' padding in ac / bc), masked after them, show theirs
    assert all(set(r["quals"][:90] + r["quals"][-90:]) <= {4, 5} for r in recs)
    assert sum("n" in r["tags"]["ac"][1] + r["tags"]["bc"][1] and 4 in r["quals"] and 5 in r["quals"] for r in recs) > len(recs) // 2


@pytest.mark.parametrize("kind", [1, 2], ids=["duplex", "codec"])
def test_one_batch_for_both_writers(kind):
    run_isolated("test_wavemu_record_writers", "check_both_writers_own_records", kind, 200, env=env(), timeout=900)


def test_duplex_records_refused_for_length():
    run_isolated("test_wavemu_record_writers", "check_duplex_refused_for_length", 60, env=env(), timeout=900)


def test_per_field_duplex_writer_methylation_build():
    run_isolated("test_wavemu_record_writers", "check_methylation_build", env=env(), timeout=1500)


def test_per_field_duplex_writer_cap_build():
    run_isolated("test_wavemu_record_writers", "check_cap_build", env=env(), timeout=900)


def test_per_field_codec_writer_both_orientations_and_quality_masks():
    run_isolated("test_wavemu_record_writers", "check_codec_orientations_and_masks", 150, env=env(), timeout=900)
