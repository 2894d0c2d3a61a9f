"""The claims of tests/volume_compare_lesion_cases.py about its own cases, checked with SciPy (no project code): the
component counts per connectivity, which cases exceed 64 components, which rest on ties, the widths with their
word-edge crossings, and the word and trip counts of the size case."""
import numpy as np
import pytest
from scipy import ndimage

import volume_compare_lesion_cases as lc

CASES = lc.cases()


def label(m, c):
    return ndimage.label(np.asarray(m), structure=ndimage.generate_binary_structure(3, 1 if c == 6 else 3))


@pytest.mark.parametrize("c", CASES, ids=lc.ids(CASES))
def test_component_counts(c):
    got = (label(c["a"], 6)[1], label(c["b"], 6)[1], label(c["a"], 26)[1], label(c["b"], 26)[1])
    assert got == c["counts"]
    assert c["exceeds"] == (max(got) > lc.MAX_LESIONS)


def test_names_are_unique_and_the_required_cases_exist():
    names = lc.ids(CASES)
    assert len(set(names)) == len(names)
    for n in ("worked_boxes", "worked_row", "width_63", "width_64", "width_65", "width_130", "diagonal", "merge", "split", "touch_one",
              "lattice", "equal_areas", "best_tie", "a_empty", "b_empty", "both_empty", "equal", "subset", "size"):
        assert n in names, n


def sizes(m, c):
    lab, n = label(m, c)
    return np.bincount(lab.ravel(), minlength=n + 1)[1:]


@pytest.mark.parametrize("c", CASES, ids=lc.ids(CASES))
def test_size_ties(c):
    """size_tie: at some connectivity some side has two components of one size."""
    tie = any(len(set(s.tolist())) < len(s) for m in (c["a"], c["b"]) for s in (sizes(m, 6), sizes(m, 26)))
    assert tie == c["size_tie"]


def pair_table(a, b, conn):
    la, na = label(a, conn)
    lb, nb = label(b, conn)
    t = np.zeros((na + 1, nb + 1), np.int64)
    both = (np.asarray(a) != 0) & (np.asarray(b) != 0)
    np.add.at(t, (la[both], lb[both]), 1)
    return t[1:, 1:]


@pytest.mark.parametrize("name", ["worked_row", "best_tie"])
def test_best_partner_ties(name):
    c = lc.case(name)
    assert c["best_tie"]
    t = pair_table(c["a"], c["b"], 6)
    col = t[:, 0]  # B's first component
    assert (col == col.max()).sum() >= 2 and col.max() > 0


def test_diagonal_differs_by_connectivity_on_both_sides():
    a6, b6, a26, b26 = lc.case("diagonal")["counts"]
    assert a6 > a26 and b6 > b26


def test_merge_split_touch_subset():
    t = pair_table(lc.case("merge")["a"], lc.case("merge")["b"], 26)
    assert t.shape == (1, 3) and (t > 0).all()
    t = pair_table(lc.case("split")["a"], lc.case("split")["b"], 26)
    assert t.shape == (3, 1) and (t > 0).all()
    c = lc.case("touch_one")
    assert int((c["a"] & c["b"]).sum()) == c["tp_vox"] == 1
    c = lc.case("subset")
    assert c["subset"] and int((c["a"] & ~c["b"] & 1).sum()) == 0 and int(c["b"].sum()) > int(c["a"].sum()) > 0
    c = lc.case("equal")
    assert np.array_equal(c["a"], c["b"]) and c["a"].any()
    for name, ea, eb in (("a_empty", True, False), ("b_empty", False, True), ("both_empty", True, True)):
        c = lc.case(name)
        assert (not c["a"].any()) == ea and (not c["b"].any()) == eb


@pytest.mark.parametrize("w", [63, 64, 65, 130])
def test_width_cases_cross_the_word_edges(w):
    c = lc.case(f"width_{w}")
    a, b = c["a"], c["b"]
    assert a.shape[2] == w == c["width"]
    edges = [e for e in (64, 128) if e < w]
    for long_m, short_m, y in ((a, b, 0), (b, a, 2)):
        row_l, row_s = long_m[0, y], short_m[0, y]
        for e in edges:
            assert row_l[e - 1] and row_l[e]  # the long run crosses the edge
            assert row_s[e - 1] and row_s[e]  # and so does a short run of the other mask, which began inside the word before
            if w - e >= 3:  # a short run ends inside the word the long run entered across the edge
                assert any(row_s[x] and not row_s[x + 1] and row_l[e - 1:x + 2].all() for x in range(e, min(e + 63, w - 1)))
    # row 4: both cross, from different starts
    assert a[0, 4, 0] == 0 and b[0, 4, 0] == 1 and a[0, 4, w - 1] == 1 and b[0, 4, w - 1] == 0


def test_lattice_fills_the_overflow_row_and_column():
    """At N = 64 the table's index N is non-zero in its row and in its column: by the order of nm03/volume_compare_lesions.h
    (more voxels first, then the earlier first voxel = SciPy's smaller label)."""
    c = lc.case("lattice")
    n = lc.MAX_LESIONS
    la, na = label(c["a"], 26)
    lb, nb = label(c["b"], 26)
    assert na > n and nb > n

    def ranks(lab, count):
        s = np.bincount(lab.ravel(), minlength=count + 1)[1:]
        order = np.lexsort((np.arange(count), -s))
        r = np.full(count + 1, n, np.int64)
        r[order[:n] + 1] = np.arange(n)
        return r

    ra, rb = ranks(la, na), ranks(lb, nb)
    both = (c["a"] != 0) & (c["b"] != 0)
    t = np.zeros((n + 1, n + 1), np.int64)
    np.add.at(t, (ra[la[both]], rb[lb[both]]), 1)
    assert t[n, :n].sum() > 0 and t[:n, n].sum() > 0 and t[n, n] == 5


def test_size_case_words_and_trips():
    c = lc.case("size")
    d, h, w = c["a"].shape
    assert (w, h, d) == (130, 40, 24) and lc.words(c) == 2880
    blocks = -(-lc.words(c) // lc.WORDS_PER_BLOCK)
    assert blocks == 12 and c["max_blocks"] == lc.SIZE_MAX_BLOCKS == (1, 5, None)
    trips = {mb: -(-blocks // min(blocks, mb or lc.MAX_BLOCKS)) for mb in c["max_blocks"]}
    assert trips == {1: 12, 5: 3, None: 1} and blocks % 5 != 0  # the last trip at 5 is partial
    # a body of each mask spans many workgroups: its largest component covers the words of more than four blocks
    for m in (c["a"], c["b"]):
        lab, n = label(m, 26)
        big = lab == (np.argmax(np.bincount(lab.ravel())[1:]) + 1)
        zs = np.flatnonzero(big.any(axis=(1, 2)))
        rows_per_block = lc.WORDS_PER_BLOCK / ((w + 63) // 64)
        assert (zs[-1] - zs[0]) * h / rows_per_block > 4
    # and the two bodies overlap, so the join's wave combining and table flush see them in several workgroups
    assert int((c["a"] & c["b"]).sum()) > 1000
