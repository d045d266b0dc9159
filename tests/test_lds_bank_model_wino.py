"""The LDS image of the Winograd trunk's operand V (k_trunk_w, net_wino.hip) in the brute-force bank model of
tools/lds_bank_model.py, for the board-half assignment of rows to N-tiles ("halves": six fragments per position) and the
row-parity one the kernel ships ("parity": four fragments F0..F3, each read once for both of its row taps).

The model's addresses are the kernel's formulas restated; wino_image_errors ties the two sides of the image together (every
read returns the channels of the tile the epilogue stored there), so a key that is conflict-free but reads the wrong tile
cannot pass."""
import importlib.util
import os

import pytest

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "lds_bank_model.py")
_spec = importlib.util.spec_from_file_location("_lds_bank_model", _PATH)
bm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bm)


@pytest.fixture(scope="module")
def cyc():
    return {m: (bm.wino_read_cycles(m), bm.wino_store_cycles(m)) for m in bm.WINO_MAPPINGS}


def test_fragment_counts():
    assert len(bm.wino_fragments("halves")) == 6 and len(bm.wino_fragments("parity")) == 4
    # F0..F3 are rows {-1,1,3,5}, {0,2,4,6}, {1,3,5,7}, {2,4,6,8}
    assert [[f(r) for r in range(4)] for f in bm.wino_fragments("parity")] == [[-1, 1, 3, 5], [0, 2, 4, 6], [1, 3, 5, 7],
                                                                                  [2, 4, 6, 8]]


@pytest.mark.parametrize("mapping", bm.WINO_MAPPINGS)
def test_every_fragment_read_is_conflict_free(cyc, mapping):
    """every fragment at every k-step, xi, position and hi / lo half: 4.0 cycles, the conflict-free cost of a ds_read_b128"""
    rd, _ = cyc[mapping]
    assert len(rd) == len(bm.wino_fragments(mapping)) * 2 * 4 * 4 * 2
    worst = max(rd.values())
    print("\n    %s: %d reads, %.2f cycles on average, worst %d" % (mapping, len(rd), sum(rd.values()) / len(rd), worst), end="")
    assert {k: v for k, v in rd.items() if v != 4} == {}


def test_epilogue_stores_cost_no_more_than_before(cyc):
    old, new = cyc["halves"][1], cyc["parity"][1]
    assert set(old) == set(new)
    print("\n    8-byte stores: halves %.2f, parity %.2f cycles" % (sum(old.values()) / len(old), sum(new.values()) / len(new)),
          end="")
    assert all(new[k] <= old[k] for k in old)


@pytest.mark.parametrize("mapping", bm.WINO_MAPPINGS)
def test_reads_return_what_the_epilogue_stored(mapping):
    assert bm.wino_image_errors(mapping) == []


def test_a_wrong_key_is_seen():
    """the checks are not vacuous: the old key under the new row assignment conflicts"""
    key = bm.wino_key
    try:
        bm.wino_key = lambda mapping, y, j: ((y & 3) * 4 + j) & 15
        assert max(bm.wino_read_cycles("parity").values()) > 4
    finally:
        bm.wino_key = key
