"""What the cases of tests/ppmd_common.py exercise in gmix_amd/csrc/gmx_ppmd.h, counted by the header's own counters
(-DGMX_PPMD_CENSUS, host build only; compiled out of the device build): every branch tests/golden/ppmd_trace.npz was
chosen for is taken by the bytes the CPU and GPU tests replay.  The lane-boundary table sizes (64, 65, 128, 129, 256
symbols) are scanned in rand256: its order-1 contexts grow through each of them, its root holds all 256."""
import numpy as np
import pytest

import ppmd_common as pc


def run(name):
    before, ns0 = pc.census()
    m = pc.HostModel(pc.CASES[name][2], pc.ARENA_MB, census=True)
    m.run(pc.case_bytes(name), want_ppm=False)
    m.close()
    after, ns1 = pc.census()
    return {k: after[k] - before[k] for k in after}, ns1 - ns0


@pytest.fixture(scope="module")
def counts():
    return {name: run(name) for name in pc.CASES}


def test_flush_only_branches(counts):
    c, _ = counts["sym3"]
    assert c["restore"] == 1
    for k in ("cutoff", "cut_free", "cut_fold", "cut_rescale", "move_up", "glue"):
        assert c[k] >= 1, (k, c)
    c, _ = counts["rand256"]
    assert c["restore"] == 1 and c["rare_null"] >= 1, c      # the allocator gives up in AllocUnitsRare
    c, _ = counts["abcd"]
    assert c["restore"] == 1 and c["cut_bin_free"] >= 1, c
    for name in ("noisy500", "e-run", "rand256_o4", "sym3_o64"):
        assert counts[name][0]["restore"] == 0, name


def test_common_branches_at_least_100_times(counts):
    total = {k: sum(counts[n][0][k] for n in counts) for k in pc.CENSUS_NAMES}
    for k in ("rescale", "rescale_zero", "rescale_fold", "full_order", "reduce_order", "expand", "bin_to_two", "shift_rare",
              "split", "bin_update"):
        assert total[k] >= 100, (k, total)
    c, _ = counts["noisy500"]
    for k in ("rescale", "rescale_zero", "rescale_fold", "full_order", "bin_update"):
        assert c[k] >= 100, (k, c)
    c, _ = counts["rand256"]
    assert c["split"] >= 100 and c["shift_rare"] >= 100, c
    # UpdateModel's `pText >= UnitsStart` exit: no input here reaches it (the allocator takes the text gap first)
    assert total["text_full"] == 0


def test_lane_boundary_table_sizes_are_scanned(counts):
    _, ns = counts["rand256"]
    for size in (64, 65, 128, 129, 256):
        assert ns[size] >= 1, (size, ns[60:70], ns[124:132])
    assert counts["sym3"][1][3] >= 1 and counts["abcd"][1][4] >= 1
