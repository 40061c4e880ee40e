"""No GPU: the closed-form pixel owner the stitch of sbbseg_segment_views_dev evaluates (csrc/region.h region_owner, through
sbbseg_debug_axis_owner) against the kept ranges of sbbseg_debug_owned_range -- what stitch_kernel's uploaded owner tables encode --
and the new names in the header and the export list."""
import os
import re

import numpy as np
import pytest

from sbb_textline_detection_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sbbseg_segment_views_dev", "sbbseg_segment_views", "sbbseg_debug_axis_owner"]


def _tile_counts(extent, tile, mid):
    """The reference's count, and the count after the dedupe rule where the last two clamped origins coincide."""
    n = -(-extent // mid)
    origin = [min(t * mid, extent - tile) for t in range(n)]
    return [n, n - 1] if n >= 2 and origin[-1] == origin[-2] else [n]


@pytest.mark.parametrize("tile,margin", [(64, 6), (224, 22), (448, 44)])
def test_axis_owner_is_the_owned_range_of_exactly_one_tile(tile, margin):
    mid = tile - 2 * margin
    deduped = 0
    for extent in range(tile, tile + 4 * mid + 1):
        for n in _tile_counts(extent, tile, mid):
            deduped += n != -(-extent // mid)
            own = _capi.host_axis_owner(extent, tile, margin, n)
            want = np.full(extent, -1, np.int64)
            owners = np.zeros(extent, np.int32)
            for t in range(n):
                origin = min(t * mid, extent - tile)
                lo, hi = _capi.owned_range(extent, tile, margin, n, t)
                q = np.arange(origin + lo, origin + hi)
                want[q] = (t << 16) | (q - origin)
                owners[q] += 1
            assert (owners == 1).all(), (extent, n, np.flatnonzero(owners != 1)[:4])
            assert np.array_equal(own, want), (extent, n, np.flatnonzero(own != want)[:4])
    assert deduped > 0                                   # (the dedupe rule applied somewhere in the sweep)


def test_axis_owner_rejects_bad_arguments():
    with pytest.raises(RuntimeError):
        _capi.host_axis_owner(100, 224, 22, 1)           # extent < tile


def test_new_names_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sbbseg.h")).read()
    lib = _capi.load_library()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _capi.EXPORTS
        assert hasattr(lib, name)
    assert "typedef struct sbbseg_view" in hdr
    assert lib.sbbseg_abi_version() == 5
