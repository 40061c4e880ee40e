"""The planes of tests/cc_planes.py hold what they claim (scipy and the oracle only: no family may pass tests/test_gpu_components.py
vacuously), and the library's HOST mirror of the box search equals the scipy oracle on every region plane -- so a disagreement of the
device with the oracle is the device's.  No GPU; the host mirror needs the built library (its contour tracer)."""
import numpy as np
import pytest
from scipy import ndimage

from oracle import stage_glue as sg
from sbb_textline_detection_amd import stages

import cc_planes

EIGHT = np.ones((3, 3), int)
FOUR = [[0, 1, 0], [1, 1, 1], [0, 1, 0]]
REGION = cc_planes.region_families()
PAGE = cc_planes.page_families()
REGION_PLANES = [(f, n) for f, planes in REGION.items() for n in planes]


def _components(mask):
    """(label plane, n, slices) of the 8-connected components of mask > 0."""
    lab, n = ndimage.label(np.asarray(mask) > 0, structure=EIGHT)
    return lab, n, ndimage.find_objects(lab)


def _runs(row):
    """[(first column, last column)] of the runs of a boolean row."""
    d = np.diff(np.concatenate(([0], row.astype(np.int8), [0])))
    return list(zip(np.nonzero(d == 1)[0].tolist(), (np.nonzero(d == -1)[0] - 1).tolist()))


def test_planes_are_small_uint8_and_named_once():
    names = [n for fam in (REGION, PAGE) for planes in fam.values() for n in planes]
    assert len(names) == len(set(names))
    sides = []
    for fam in (REGION, PAGE):
        for planes in fam.values():
            for name, p in planes.items():
                assert p.dtype == np.uint8 and p.ndim == 2 and p.flags.c_contiguous, name
                assert max(p.shape) <= 520, (name, p.shape)
                sides.append(max(p.shape))
    assert sorted(sides)[len(sides) // 2] < 300                                    # most sides well under 300
    again = cc_planes._grids()                                                     # seeded: the same planes every time
    assert all(np.array_equal(again[n], REGION["grids"][n]) for n in again)
    cells = {(p.shape[0] // s, p.shape[1] // s) for p in REGION["grids"].values() for s in (6, 7, 8) if p.shape[0] % s == 0 and p.shape[1] % s == 0}
    assert cells >= {(11, 40), (30, 12)} and len(REGION["grids"]) == 9             # both aspect ratios, three fills each
    assert {p.shape for p in REGION["narrow"].values()} >= {(3, 40), (40, 4)}
    assert {p.shape for p in PAGE["chunks"].values()} >= {(1, 200), (2, 129), (200, 1), (40, 63), (40, 64), (40, 65), (40, 128)}


def test_diagonal_family_is_joined_through_corners_only():
    for name, parts in (("diag_down_right", 2), ("diag_down_left", 2), ("zigzag5", 5)):
        m = cc_planes.page_mask(PAGE["diagonal"][name]) > 0
        assert ndimage.label(m, structure=EIGHT)[1] == 1, name
        assert ndimage.label(m, structure=FOUR)[1] == parts, name
    # both diagonal directions: the lower blob's first pixel has its only upper neighbour at NW in one plane, at NE in the other
    for name, dx in (("diag_down_right", -1), ("diag_down_left", 1)):
        m = cc_planes.page_mask(PAGE["diagonal"][name]) > 0
        y = 45 - 12                                                                # the lower blob's first row
        xs = np.nonzero(m[y])[0]
        above = [x for x in xs if m[y - 1, x]]
        assert not above, name                                                     # no N link
        diag = [x for x in xs if 0 <= x + dx < m.shape[1] and m[y - 1, x + dx]]
        assert len(diag) == 1, name


def test_lattice_family_has_over_250_equal_components():
    for name in ("lattice_equal", "lattice_one_apart", "lattice_notched"):
        lab, n, slices = _components(cc_planes.page_mask(PAGE["lattice"][name]))
        assert n == 289, name
        sizes = [(s[0].stop - s[0].start, s[1].stop - s[1].start) for s in slices]
        assert max(sizes.count(v) for v in set(sizes)) >= 252, name
    lab, n, slices = _components(cc_planes.page_mask(PAGE["lattice"]["lattice_one_apart"]))
    areas = sorted(sg.outer_contour_area2(lab[sl] == k + 1) for k, sl in enumerate(slices))
    assert areas[-1] - areas[-2] == 2 * 24 and areas[0] == areas[-2]               # the winner leads by one cell column
    # notched: no holes, so the device's cell count is each blob's exact area, and every blob's bounding-box bound lies above it:
    # all 288 others stay undecided rivals of the device's best -- more than the kCcMaxRivals = 250 it can list
    lab, n, slices = _components(cc_planes.page_mask(PAGE["lattice"]["lattice_notched"]))
    lower = [cc_planes.cell_area2(lab[sl] == k + 1) for k, sl in enumerate(slices)]
    upper = [2 * (sl[0].stop - sl[0].start - 1) * (sl[1].stop - sl[1].start - 1) for sl in slices]
    assert sum(1 for u in upper if u > max(lower)) - 1 >= 251


def test_rival_plane_hides_the_winner_among_more_rivals_than_the_device_lists():
    """rivals_ring_last: the device's best (largest cell count; ties to the last) is NOT the component with the largest contour area, that
    one is the last root in raster order, and more than 250 components have a bounding-box bound above the best cell count."""
    lab, n, slices = _components(cc_planes.region_mask(REGION["rivals"]["rivals_ring_last"]))
    assert n == 289
    lower = [cc_planes.cell_area2(lab[sl] == k + 1) for k, sl in enumerate(slices)]
    exact = [sg.outer_contour_area2(lab[sl] == k + 1) for k, sl in enumerate(slices)]
    upper = [2 * (sl[0].stop - sl[0].start - 1) * (sl[1].stop - sl[1].start - 1) for sl in slices]
    best = max(range(n), key=lambda k: (lower[k], k))
    winner = max(range(n), key=lambda k: (exact[k], k))
    assert (best, winner) == (0, n - 1)                                            # scipy numbers by first pixel in raster order
    assert (lower[best], exact[best], lower[winner], exact[winner]) == (2 * 182, 2 * 182, 2 * 162, 2 * 196)
    rivals = [k for k in range(n) if k != best and upper[k] > lower[best]]
    assert len(rivals) > 251 and winner in rivals
    assert sorted(exact)[-3] < 2 * 182                                             # everything else is smaller than both


def test_at_least_eight_planes_drop_an_island_in_a_hole():
    with_islands = []
    for fam, name in REGION_PLANES:
        n = _components(cc_planes.region_mask(REGION[fam][name]))[1]
        kept = len(cc_planes.oracle_region_boxes(name, 0.0, 1.0))                   # no area bound: only islands are dropped
        assert kept <= n
        if kept < n:
            with_islands.append(name)
    assert len(with_islands) >= 8, with_islands
    # nested several deep: of the closed rings only the outermost has no parent
    lab, n, _ = _components(cc_planes.region_mask(REGION["rings"]["rings_s7"]))
    assert n == 5 and len(cc_planes.oracle_region_boxes("rings_s7", 0.0, 1.0)) == 1
    assert len(cc_planes.oracle_region_boxes("rings_edges_s6", 0.0, 1.0)) == 1
    m = cc_planes.region_mask(REGION["rings"]["rings_edges_s6"]) > 0
    assert m[0].all() and m[-1].all() and m[:, 0].all() and m[:, -1].all()          # ... and touches all four plane edges


def test_a_one_cell_channel_changes_who_is_parentless():
    closed = cc_planes.oracle_region_boxes("rings_s7", 0.0, 1.0)
    channel = cc_planes.oracle_region_boxes("rings_channel", 0.0, 1.0)
    half = cc_planes.oracle_region_boxes("rings_half_channel", 0.0, 1.0)
    assert (len(closed), len(half), len(channel)) == (1, 3, 5)
    for name in ("rings_s7", "rings_channel", "rings_half_channel"):
        assert _components(cc_planes.region_mask(REGION["rings"][name]))[1] == 5, name


def test_chunk_family_has_runs_over_and_from_column_64():
    over, from64, twice, ends = [], [], [], set()
    for name, p in PAGE["chunks"].items():
        m = cc_planes.page_mask(p) > 0
        for y in range(m.shape[0]):
            for a, b in _runs(m[y]):
                if a <= 63 and b >= 64:
                    over.append(name)
                if a == 64:
                    from64.append(name)
                if a < 64 and b >= 128:
                    twice.append(name)
                if b == m.shape[1] - 1:
                    ends.add(b)
    assert over and from64 and twice
    assert {"chunk_1x200_51_76", "chunk_40x128_51_76", "chunk_40x65_52"} <= set(over)
    assert {"chunk_1x200_76", "chunk_2x129_76", "chunk_40x128_76"} <= set(from64)
    assert ends >= {0, 62, 63, 64, 127, 128, 199}                                  # runs that end with the row, either side of a chunk's end
    column = cc_planes.page_mask(PAGE["chunks"]["chunk_200x1_51_76"])[:, 0] > 0     # width 1: the same runs, downwards
    assert (39, 88) in _runs(column)


def test_paths_are_one_component_of_many_rows():
    for name in ("spiral", "serpentine", "comb", "comb_upside_down"):
        m = cc_planes.region_mask(REGION["paths"][name])
        lab, n, slices = _components(m)
        assert n == 1, name
        assert slices[0][0].stop - slices[0][0].start >= 100, name
        runs = sum(len(_runs(row > 0)) for row in m)
        assert runs >= (100 if name == "serpentine" else 1000), (name, runs)       # a run per row at the least; the others a dozen per row
    assert cc_planes.spiral_grid(49)[1] >= 4 * 12                                  # twelve times round
    teeth = max(len(_runs(row > 0)) for row in cc_planes.region_mask(REGION["paths"]["comb"]))
    assert teeth >= 20
    m = cc_planes.region_mask(REGION["paths"]["comb"]) > 0
    assert len(_runs(m[-1])) == 1 and len(_runs(m[-7])) == teeth                   # joined along the bottom rows only
    m = cc_planes.region_mask(REGION["interleaved"]["checker"]) > 0                # the region path's diagonal links
    assert ndimage.label(m, structure=EIGHT)[1] == 1 and ndimage.label(m, structure=FOUR)[1] == 240


def test_every_region_family_has_a_plane_of_ten_boxes():
    for fam, planes in REGION.items():
        most = max(len(cc_planes.oracle_region_boxes(n, 0.0, 1.0)) for n in planes)
        assert most >= 10, (fam, most)


def test_interior_windows_split_the_components():
    """The per-plane window of the GPU test drops something and keeps something wherever a plane has components of two sizes."""
    split = 0
    for fam, name in REGION_PLANES:
        lo, hi = cc_planes.interior_window(name)
        everything = cc_planes.oracle_region_boxes(name, 0.0, 1.0)
        inside = cc_planes.oracle_region_boxes(name, lo, hi)
        assert 0.0 < lo <= hi < 1.0 or not everything, name
        if everything:
            assert inside, name
        if len(set(sg.text_region_contour_areas(REGION[fam][name], 1, 0.0, 1.0))) >= 2:
            assert 0 < len(inside) < len(everything), name
            split += 1
    assert split >= 10


@pytest.mark.parametrize("family", list(REGION))
def test_host_mirror_equals_the_scipy_oracle(family):
    for name, plane in REGION[family].items():
        for m in (0.0, 1e-5):
            assert stages.host_text_region_boxes(plane, 1, min_area=m) == cc_planes.oracle_region_boxes(name, m, 1.0), (name, m)      # slopes_ref.oracle_boxes, shared
        lo, hi = cc_planes.interior_window(name)
        assert stages.host_text_region_boxes(plane, 1, min_area=lo, max_area=hi) == cc_planes.oracle_region_boxes(name, lo, hi), name


@pytest.mark.parametrize("family", list(PAGE))
def test_host_page_box_equals_the_scipy_oracle(family):
    for name, plane in PAGE[family].items():
        assert stages.host_page_box(plane) == sg.page_box(plane), name
    assert sg.page_box(PAGE["empty"]["empty_64x64"]) == ((0, 0, 0, 0), 0)
