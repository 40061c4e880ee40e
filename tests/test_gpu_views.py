"""-m gpu: sbbseg_segment_views_dev -- tiles of differently sized pages and crops pooled into shared launches -- against the one-view
entry points on the same handle.  Every comparison is np.array_equal: the network kernels are bit-identical per tile whatever else is in
the batch, so the new ingest, region-table and stitch kernels (geometry per tile, owner in closed form) must reproduce the label planes
and thresholds byte for byte.

The 224 x 224 model (margin 22, mid 180) is the smallest whose plan has owned-region levels.  Extents: 224 = one tile, 360 = an exact
multiple of mid, 404 = the last residue at which the clamped last tile repeats (the dedupe rule drops it), 405 = the first at which it
does not, 225 / 361 = one pixel past a boundary, 540 = three tiles."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_common import make_model  # noqa: E402
from sbb_textline_detection_amd import _capi  # noqa: E402
from sbb_textline_detection_amd.stages import scaled_size  # noqa: E402
from sbb_textline_detection_amd.synthetic import synthetic_page  # noqa: E402

MAX_BATCH = 24
MIXED = [(224, 224), (404, 540), (360, 540), (361, 405), (540, 361), (405, 225)]          # pairwise different (H, W)
ONE_CHUNK = [(224, 224), (225, 360), (360, 225), (404, 360), (360, 404), (225, 225)]       # 21 tiles with the dedupe rule


def _tiles(h, w, dedupe, tile=224):
    """Tiles of an h x w page: the reference's grid, less the repeated clamped tile per axis under the dedupe rule."""
    xy, nx, ny = _capi.tile_grid(h, w, tile, tile)
    if dedupe:
        xs, ys = sorted(set(xy[:, 0].tolist())), sorted(set(xy[:, 1].tolist()))
        nx, ny = len(xs), len(ys)
    return nx * ny


def _chunks(n_tiles, max_batch=MAX_BATCH):
    n_chunks = -(-n_tiles // max_batch)
    chunk = -(-n_tiles // n_chunks)
    return [(a, min(a + chunk, n_tiles)) for a in range(0, n_tiles, chunk)]


@pytest.fixture(scope="module", params=["f16x3", "f16"])
def model224(request):
    cfg, w, g, model = make_model(2, 224, 224, seed=5, precision=request.param, max_batch=MAX_BATCH, calib_hw=160)
    yield model
    model.release()


@pytest.fixture(scope="module")
def torch_pages():
    import torch
    out = {}
    for hw in sorted(set(MIXED + ONE_CHUNK)):
        out[hw] = torch.from_numpy(synthetic_page(hw[0], hw[1], seed=hw[0] * 3 + hw[1])).cuda()
    return out


def _full_view(t, d_out):
    h, w = t.shape[:2]
    return (t.data_ptr(), h, w, h, w, (0, 0, w, h), False, d_out.data_ptr())


def _planes(sizes):
    import torch
    return [torch.full(hw, 9, dtype=torch.uint8, device="cuda") for hw in sizes]


def _page_by_page(ctx, pages, sizes):
    outs = _planes(sizes)
    for hw, o in zip(sizes, outs):
        ctx.segment_page_dev(pages[hw].data_ptr(), hw[0], hw[1], o.data_ptr())
    ctx.synchronize()
    return [o.cpu().numpy() for o in outs]


def _pooled(ctx, pages, sizes):
    outs = _planes(sizes)
    ctx.segment_views_dev([_full_view(pages[hw], o) for hw, o in zip(sizes, outs)])
    ctx.synchronize()
    return [o.cpu().numpy() for o in outs]


def test_the_mixed_set_exercises_the_chunk_boundaries():
    """(no GPU work) what the mixed-page test relies on, from the tile grids: a total that is no multiple of the chunk, a chunk that spans at
    least three views, a view that spans two chunks -- with and without the dedupe rule; and two lanes get work in both."""
    assert len(set(MIXED)) == len(MIXED) and (224, 224) in MIXED and (404, 540) in MIXED
    for dedupe in (True, False):
        counts = [_tiles(h, w, dedupe) for h, w in MIXED]
        first = np.concatenate([[0], np.cumsum(counts)])
        total = int(first[-1])
        chunks = _chunks(total)
        assert len(chunks) >= 2 and total % (chunks[0][1] - chunks[0][0]) != 0, (dedupe, total, chunks)
        assert all(b - a >= 16 for a, b in chunks[:-1]), chunks
        spans = [sum(1 for k in range(len(MIXED)) if first[k] < b and first[k + 1] > a) for a, b in chunks]
        assert max(spans) >= 3, (dedupe, spans)
        cut = [sum(1 for a, b in chunks if first[k] < b and first[k + 1] > a) for k in range(len(MIXED))]
        assert max(cut) >= 2, (dedupe, cut)
    assert _tiles(404, 540, True) == 6 and _tiles(404, 540, False) == 9 and _tiles(405, 540, True) == 9 and _tiles(224, 224, True) == 1


def test_mixed_plain_pages_equal_page_by_page(model224, torch_pages):
    ctx = model224.ctx
    assert ctx.owned_region_levels() >= 3
    try:
        for dedupe in (True, False):
            ctx.set_dedupe(dedupe)
            for lanes in (1, 2):
                ctx.set_lanes(lanes)
                ctx.set_owned_regions(0)
                ref = _page_by_page(ctx, torch_pages, MIXED)
                assert all(0.01 < float(r.mean()) < 0.99 for r in ref)
                before = ctx.forwards()
                whole = _pooled(ctx, torch_pages, MIXED)
                assert ctx.forwards() - before == sum(_tiles(h, w, dedupe) for h, w in MIXED)
                ctx.poison_activations(0xFF)
                ctx.set_owned_regions(1)
                owned = _pooled(ctx, torch_pages, MIXED)
                for hw, r, a, b in zip(MIXED, ref, whole, owned):
                    assert np.array_equal(a, r), (hw, dedupe, lanes, "whole tiles", int((a != r).sum()))
                    assert np.array_equal(b, r), (hw, dedupe, lanes, "owned regions", int((b != r).sum()))
    finally:
        ctx.set_dedupe(True)
        ctx.set_lanes(2)
        ctx.set_owned_regions(1)


def test_more_views_than_one_group_holds(model224, torch_pages):
    """7 x the mixed set = 217 tiles: more than the eight chunks a group takes, so the call runs two groups over one scratch buffer."""
    ctx = model224.ctx
    ref = _page_by_page(ctx, torch_pages, MIXED)
    sizes = MIXED * 7
    assert sum(_tiles(h, w, True) for h, w in sizes) > 8 * MAX_BATCH
    got = _pooled(ctx, torch_pages, sizes)
    for k, g in enumerate(got):
        assert np.array_equal(g, ref[k % len(MIXED)]), k


def test_crops_rescale_binarise_equal_segment_crop(model224):
    import torch
    ctx = model224.ctx
    stored = [synthetic_page(300, 260, seed=21), synthetic_page(410, 333, seed=22)]
    scaled = [scaled_size(*p.shape[:2]) for p in stored]
    assert scaled == [(2800, 2426), (2800, 2274)]
    # (page, box (x, y, w, h) on the upscaled page, binarise): odd corners; the second touches page 0's right and bottom edge
    views = [(0, (101, 203, 360, 540), True), (0, (2426 - 405, 2800 - 361, 405, 361), False),
             (1, (301, 77, 540, 225), False), (1, (1501, 1001, 361, 404), True)]
    assert all(x % 2 == 1 and y % 2 == 1 for _, (x, y, w, h), _ in views)
    d_pages = [torch.from_numpy(p).cuda() for p in stored]
    want, want_thr = [], []
    for pg, box, binarise in views:
        out = torch.full((box[3], box[2]), 9, dtype=torch.uint8, device="cuda")
        thr = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        ctx.segment_crop_dev(d_pages[pg].data_ptr(), stored[pg].shape[0], stored[pg].shape[1], scaled[pg][0], scaled[pg][1], box, binarise,
                             out.data_ptr(), thr.data_ptr())
        ctx.synchronize()
        want.append(out.cpu().numpy())
        want_thr.append(int(thr.item()))
    outs = [torch.full((box[3], box[2]), 9, dtype=torch.uint8, device="cuda") for _, box, _ in views]
    thrs = torch.full((len(views),), -1, dtype=torch.int32, device="cuda")
    ctx.segment_views_dev([(d_pages[pg].data_ptr(), stored[pg].shape[0], stored[pg].shape[1], scaled[pg][0], scaled[pg][1], box, binarise,
                            outs[k].data_ptr(), thrs[k:].data_ptr()) for k, (pg, box, binarise) in enumerate(views)])
    ctx.synchronize()
    got_thr = thrs.cpu().numpy().tolist()
    for k, (pg, box, binarise) in enumerate(views):
        assert np.array_equal(outs[k].cpu().numpy(), want[k]), (k, box)
        assert got_thr[k] == want_thr[k] and (0 <= got_thr[k] <= 255) == binarise, (k, got_thr, want_thr)
    # the host form: pages uploaded once each, planes and thresholds back; three identical channels on request
    host = model224.segment_views([(stored[pg], scaled[pg][0], scaled[pg][1], box, binarise) for pg, box, binarise in views])
    host3 = ctx.segment_views([(stored[pg], scaled[pg][0], scaled[pg][1], box, binarise) for pg, box, binarise in views], channels=3)
    for k, (pg, box, binarise) in enumerate(views):
        assert np.array_equal(host[k][0], want[k]) and host[k][1] == (want_thr[k] if binarise else None), k
        assert host3[k][0].shape == want[k].shape + (3,) and all(np.array_equal(host3[k][0][:, :, ch], want[k]) for ch in range(3)), k
        assert host3[k][1] == host[k][1]


def test_f32_handle_without_owned_levels():
    import torch
    cfg, w, g, model = make_model(2, 64, 64, seed=2, precision="f32", max_batch=MAX_BATCH)
    try:
        ctx = model.ctx
        assert ctx.owned_region_levels() == 0
        sizes = [(64, 64), (130, 117), (200, 90)]
        pages = {hw: torch.from_numpy(synthetic_page(hw[0], hw[1], seed=hw[1])).cuda() for hw in sizes}
        ref = _page_by_page(ctx, pages, sizes)
        got = _pooled(ctx, pages, sizes)
        for hw, r, a in zip(sizes, ref, got):
            assert np.array_equal(a, r), hw
    finally:
        model.release()


def test_launch_structure(model224, torch_pages):
    """Six views in one chunk: one ingest, one region-table build and one stitch launch on one lane; two of the first two on two lanes."""
    ctx = model224.ctx
    n = sum(_tiles(h, w, True) for h, w in ONE_CHUNK)
    assert 16 <= n <= MAX_BATCH
    try:
        for lanes, owned, want in ((1, 1, 3), (1, 0, 2), (2, 1, 5), (2, 0, 3)):
            ctx.set_lanes(lanes)
            ctx.set_owned_regions(owned)
            before = ctx.views_launches()
            _pooled(ctx, torch_pages, ONE_CHUNK)
            assert ctx.views_launches() - before == want, (lanes, owned)
    finally:
        ctx.set_lanes(2)
        ctx.set_owned_regions(1)


def test_bad_views_fail_whole_and_name_the_view(model224, torch_pages):
    import torch
    ctx = model224.ctx
    page = torch_pages[(404, 540)]
    good = torch.full((404, 540), 9, dtype=torch.uint8, device="cuda")
    other = torch.full((404, 540), 9, dtype=torch.uint8, device="cuda")
    ok = _full_view(page, good)
    before, forwards = ctx.views_launches(), ctx.forwards()
    with pytest.raises(RuntimeError, match="n_views 0"):
        ctx.segment_views_dev([])
    with pytest.raises(RuntimeError, match=r"view 1: .*smaller than the model input"):
        ctx.segment_views_dev([ok, (page.data_ptr(), 404, 540, 404, 540, (0, 0, 540, 223), False, other.data_ptr())])
    with pytest.raises(RuntimeError, match=r"view 2: .*leaves the 404x540 page"):
        ctx.segment_views_dev([ok, ok, (page.data_ptr(), 404, 540, 404, 540, (317, 0, 224, 224), False, other.data_ptr())])
    with pytest.raises(RuntimeError, match=r"view 1: null"):
        ctx.segment_views_dev([ok, (page.data_ptr(), 404, 540, 404, 540, (0, 0, 540, 404), False, 0)])
    ctx.synchronize()
    assert ctx.views_launches() == before and ctx.forwards() == forwards          # nothing was launched
    assert int((good != 9).sum().item()) == 0
    ref = _page_by_page(ctx, torch_pages, [(404, 540)])[0]
    ctx.segment_views_dev([ok])
    ctx.synchronize()
    assert np.array_equal(good.cpu().numpy(), ref)


def test_run_pages_equals_run_page_by_page(tmp_path):
    """Three stored images of different sizes through three models built the way the other stage tests build theirs.  The last image is
    40 pixels wide: upscaled to 2800 x 186 its page box cannot hold the layout model's 224 x 224 input, so run() gives it regions = None,
    textlines = None (main.py:278-285 under 2089-2091) -- and it must not fail the pooled call of the other two."""
    from sbb_textline_detection_amd import clear_session, stages
    from sbb_textline_detection_amd.model import load_model
    from sbb_textline_detection_amd.weights import save_sbbw
    from tools.synth_model import calibrated_model
    specs = {"model_page_mixed_best": 2, "model_strukturerkennung": 4, "model_textline_new": 2}      # main.py:58-60
    for name, classes in specs.items():
        cfg, w = calibrated_model(classes, 224, 224, seed=classes)
        save_sbbw(str(tmp_path / (name + ".sbbw")), cfg, w)
    st = stages.InferenceStages(*[str(tmp_path / (n + ".h5")) for n in specs], model_kwargs={"max_batch": 16})
    # (narrow strips keep the test short: every image is upscaled to 2800 rows, 2800 x 280 / 2800 x 403 / 2800 x 186 here)
    images = [np.ascontiguousarray(synthetic_page(h, 400, seed=s)[:, :w]) for h, w, s in ((600, 60, 6), (520, 75, 9), (600, 40, 1))]
    try:
        small = []
        for img in images:
            st.get_image_and_scales(img)
            _, box, _ = st.page_box_only()
            small.append(box[2] < 224 or box[3] < 224)
        assert small == [False, False, True], small
        want = [st.run(img) for img in images]
        layout = load_model(str(tmp_path / "model_strukturerkennung.h5"), max_batch=16)
        before = layout.ctx.views_launches()
        got = st.run_pages(images)
        assert layout.ctx.views_launches() > before                          # (the pooled path ran, not the loop)
        assert len(got) == len(want)
        for k, (a, b) in enumerate(zip(got, want)):
            assert a[3] == b[3], k
            for x, y in zip(a[:3], b[:3]):
                assert (x is None) == (y is None), k
                if x is not None:
                    assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), k
        assert [g[1] is None for g in got] == small and got[2][2] is None
        assert got[0][2] is not None and got[1][2] is not None               # (the textline model ran on the pooled crops too)
    finally:
        clear_session()
