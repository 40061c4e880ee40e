"""-m gpu: sbbseg_segment_whole_views_dev / sbbseg_extract_page_boxes_dev -- the whole-image branch for many pages in shared launches --
against the one-page entry points on the same handle with split-K off.  Every comparison is np.array_equal: the network kernels give a
patch the same bits whatever else is in the batch (tests/test_gpu_views.py rests on the same fact), so the new ingest and label-resize
kernels must reproduce the planes byte for byte.

The model is the 224 x 224 two-class net of tests/test_gpu_views.py (make_model(2, 224, 224, seed=5, calib_hw=160): calibrated once here,
the handles of both precisions and of every max_batch are built from the same config and weights)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from gpu_common import exact_label_check  # noqa: E402
from oracle import keras_forward as kf  # noqa: E402
from sbb_textline_detection_amd.model import SegModel  # noqa: E402
from sbb_textline_detection_amd.synthetic import synthetic_page  # noqa: E402
from tools.synth_model import calibrated_model  # noqa: E402

# (stored, page after get_image_and_scales, label plane): pairwise different stored sizes; views 0, 2, 3 are rescaled, 1 and 4 are not; the
# planes: an odd width (333 x 257, as test_whole_image_branch_matches_oracle's 840 x 624 is no multiple of anything), the model's own
# size, the page's size (twice), and 120 x 401
VIEWS = [((150, 100), (300, 200), (333, 257)),
         ((224, 224), (224, 224), (224, 224)),
         ((301, 211), (361, 253), (361, 253)),
         ((97, 333), (194, 666), (120, 401)),
         ((260, 180), (260, 180), (260, 180))]
PAGE_SIZED = [(s, p, p) for s, p, _ in VIEWS]          # extract_page's use: the mask has the page's size
FILL = 9


@pytest.fixture(scope="module")
def net():
    return calibrated_model(2, 224, 224, seed=5, calib_hw=160)


@pytest.fixture(scope="module", params=["f16x3", "f16"])
def handles(request, net):
    """max_batch -> handle of the module's precision, built on first use"""
    cfg, w = net
    made = {}

    def get(max_batch):
        if max_batch not in made:
            made[max_batch] = SegModel(cfg, w, device=0, max_batch=max_batch, precision=request.param)
        return made[max_batch]
    get.precision = request.param
    yield get
    for m in made.values():
        m.release()


@pytest.fixture(scope="module")
def pages():
    import torch
    host = [synthetic_page(s[0], s[1], seed=3 * s[0] + s[1]) for s, _, _ in VIEWS]
    return host, [torch.from_numpy(p).cuda() for p in host]


def _per_page(ctx, host, views, ksplit=False):
    """the one-page entry point on every view, split-K off (the contract's reference) unless asked otherwise"""
    ctx.set_ksplit(ksplit)
    try:
        return [ctx.segment_whole_scaled(pg, p[0], p[1], o[0], o[1]) for pg, (_, p, o) in zip(host, views)]
    finally:
        ctx.set_ksplit(True)


class Planes:
    """label planes carved out of one buffer filled with 9: the first starts at an odd byte, the gaps between them are odd too"""

    def __init__(self, sizes):
        import torch
        self.sizes, self.at, end = list(sizes), [], 7
        for h, w in self.sizes:
            self.at.append(end)
            end += h * w + 13
        self.buf = torch.full((end + 64,), FILL, dtype=torch.uint8, device="cuda")
        assert self.at[0] % 2 == 1 and (len(self.at) == 1 or len({a % 16 for a in self.at}) > 1)

    def ptr(self, k):
        return self.buf.data_ptr() + self.at[k]

    def read(self):
        """(planes, every byte outside them is still 9)"""
        flat = self.buf.cpu().numpy()
        outside = np.ones(flat.shape, bool)
        got = []
        for (h, w), a in zip(self.sizes, self.at):
            got.append(flat[a:a + h * w].reshape(h, w).copy())
            outside[a:a + h * w] = False
        return got, bool((flat[outside] == FILL).all())


def _views(dev, views, planes, idx=None):
    idx = range(len(views)) if idx is None else idx
    return [(dev[k % len(dev)].data_ptr(),) + views[k][0] + views[k][1] + views[k][2] + (planes.ptr(q),) for q, k in enumerate(idx)]


def test_five_views_equal_the_one_page_calls(handles, pages, net):
    host, dev = pages
    model = handles(8)
    ctx = model.ctx
    want = _per_page(ctx, host, VIEWS)
    assert all(0.01 < float(w.mean()) < 0.99 for w in want)                    # (both classes occur: the planes say something)
    planes = Planes([o for _, _, o in VIEWS])
    ctx.segment_whole_views_dev(_views(dev, VIEWS, planes))
    ctx.synchronize()
    got, clean = planes.read()
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (k, int((g != w).sum()))
    assert clean, "a byte outside the planes was written"
    # the host form
    hosted = model.segment_whole_views([(pg, p[0], p[1], o[0], o[1]) for pg, (_, p, o) in zip(host, VIEWS)])
    assert all(np.array_equal(a, b) for a, b in zip(hosted, want))
    if handles.precision == "f16x3":
        # view 1 is the model's own size end to end: its plane is the argmax itself, held to the oracle as test_whole_image_branch_matches_oracle
        # holds the one-page call (labels equal wherever the oracle's top-2 margin exceeds EXACT_MARGIN)
        cfg, w = net
        ref = kf.OracleModel(cfg, w).predict((host[1] / 255.0)[None].astype(np.float32))[0]
        mism, outside = exact_label_check(ref, np.eye(2, dtype=np.float32)[got[1]])
        assert outside == 0, (mism, outside)


@pytest.mark.parametrize("max_batch,n_views,chunks", [(4, 9, [3, 3, 3]), (2, 3, [2, 1])])
def test_chunking(handles, pages, max_batch, n_views, chunks):
    host, dev = pages
    ctx = handles(max_batch).ctx
    want = _per_page(ctx, host, VIEWS)
    idx = [k % len(VIEWS) for k in range(n_views)]
    out = {}
    for ksplit in (True, False):
        ctx.set_ksplit(ksplit)
        try:
            planes = Planes([VIEWS[k][2] for k in idx])
            launches, forwards = ctx.whole_launches(), ctx.forwards()
            ctx.segment_whole_views_dev(_views(dev, VIEWS, planes, idx))
            ctx.synchronize()
            assert ctx.whole_launches() - launches == 2 * len(chunks)          # one ingest + one label resize per chunk, 1 view or 3
            assert ctx.forwards() - forwards == n_views
        finally:
            ctx.set_ksplit(True)
        out[ksplit], clean = planes.read()
        assert clean
        for q, k in enumerate(idx):                                            # (the one-view chunk of 2 + 1 did not split)
            assert np.array_equal(out[ksplit][q], want[k]), (ksplit, q, k)
    assert all(np.array_equal(a, b) for a, b in zip(out[True], out[False]))


def test_one_view_takes_the_one_page_route(handles, pages):
    host, dev = pages
    ctx = handles(8).ctx
    for ksplit in (True, False):
        want = _per_page(ctx, host, VIEWS, ksplit=ksplit)
        ctx.set_ksplit(ksplit)
        try:
            for k in (0, 1, 3):
                planes = Planes([VIEWS[k][2]])
                launches, forwards = ctx.whole_launches(), ctx.forwards()
                ctx.segment_whole_views_dev(_views(dev, VIEWS, planes, [k]))
                ctx.synchronize()
                assert ctx.whole_launches() - launches == 2 and ctx.forwards() - forwards == 1
                got, clean = planes.read()
                assert clean and np.array_equal(got[0], want[k]), (ksplit, k)
        finally:
            ctx.set_ksplit(True)


def test_launch_structure(handles, pages):
    host, dev = pages
    ctx = handles(8).ctx
    for idx in ([0, 1], [0, 1, 2, 3], [4, 3, 2, 1, 0, 1, 2, 3]):               # one chunk of 2, 4 and 8 views
        planes = Planes([VIEWS[k][2] for k in idx])
        launches, forwards = ctx.whole_launches(), ctx.forwards()
        ctx.segment_whole_views_dev(_views(dev, VIEWS, planes, idx))
        ctx.synchronize()
        assert ctx.whole_launches() - launches == 2, idx
        assert ctx.forwards() - forwards == len(idx), idx


def test_bad_views_fail_whole_and_name_the_view(handles, pages):
    host, dev = pages
    ctx = handles(8).ctx
    idx = [0, 1, 2]
    planes = Planes([VIEWS[k][2] for k in idx])
    good = _views(dev, VIEWS, planes, idx)
    launches, forwards = ctx.whole_launches(), ctx.forwards()
    d_page, sh, sw, ph, pw, oh, ow, d_out = good[2]
    for bad in ((0, sh, sw, ph, pw, oh, ow, d_out), (d_page, sh, sw, ph, pw, oh, ow, 0), (d_page, sh, sw, ph, pw, 0, ow, d_out),
                (d_page, sh, 0, ph, pw, oh, ow, d_out), (d_page, sh, sw, -1, pw, oh, ow, d_out)):
        with pytest.raises(RuntimeError, match=r"view 2: (null|bad size)"):
            ctx.segment_whole_views_dev(good[:2] + [bad])
    with pytest.raises(RuntimeError, match="n_views 0"):
        ctx.segment_whole_views_dev([])
    ctx.synchronize()
    assert ctx.whole_launches() == launches and ctx.forwards() == forwards      # nothing was launched
    got, clean = planes.read()
    assert clean and all(int((g != FILL).sum()) == 0 for g in got)
    want = _per_page(ctx, host, VIEWS)
    ctx.segment_whole_views_dev(good)
    ctx.synchronize()
    got, clean = planes.read()
    assert clean and all(np.array_equal(got[q], want[k]) for q, k in enumerate(idx))


def _box_views(dev, planes=None):
    return [(dev[k].data_ptr(),) + s + p + o + (planes.ptr(k) if planes else 0,) for k, (s, p, o) in enumerate(PAGE_SIZED)]


def test_page_boxes_equal_the_one_page_calls(handles, pages):
    import torch
    host, dev = pages
    ctx = handles(8).ctx
    want = []
    ctx.set_ksplit(False)
    try:
        for k, (s, p, _) in enumerate(PAGE_SIZED):
            d_mask = torch.full(p, FILL, dtype=torch.uint8, device="cuda")
            box, px = ctx.extract_page_box_dev(dev[k].data_ptr(), s[0], s[1], p[0], p[1], d_mask.data_ptr())
            want.append((box, px, d_mask.cpu().numpy()))
    finally:
        ctx.set_ksplit(True)
    assert all(px > 0 and box[2] > 0 and box[3] > 0 for box, px, _ in want)
    planes = Planes([p for _, p, _ in PAGE_SIZED])
    launches = ctx.whole_launches()
    got = ctx.extract_page_boxes_dev(_box_views(dev, planes))
    assert ctx.whole_launches() - launches == 2
    masks, clean = planes.read()
    assert clean
    for k, ((box, px), (wbox, wpx, wmask)) in enumerate(zip(got, want)):
        assert box == wbox and px == wpx, (k, box, wbox, px, wpx)
        assert np.array_equal(masks[k], wmask), k
    assert ctx.extract_page_boxes_dev(_box_views(dev)) == got                  # the masks in library scratch: the same boxes
    with pytest.raises(RuntimeError, match=r"view 0: the mask 333x257 must have the page's size 300x200"):
        ctx.extract_page_boxes_dev([(dev[0].data_ptr(),) + VIEWS[0][0] + VIEWS[0][1] + VIEWS[0][2] + (0,)])


def test_page_boxes_of_empty_masks(handles, pages, net):
    """a border model whose head bias forces class 0: every mask is empty, every box {0, 0, 0, 0} with 0 pixels, and the call succeeds"""
    host, dev = pages
    cfg, w = net
    w0 = dict(w)
    last_bias = [k for k in w0 if k.endswith("/bias:0")][-1]
    w0[last_bias] = np.array([1.0e4, -1.0e4], w0[last_bias].dtype)
    model = SegModel(cfg, w0, device=0, max_batch=8, precision=handles.precision)
    try:
        planes = Planes([p for _, p, _ in PAGE_SIZED])
        got = model.ctx.extract_page_boxes_dev(_box_views(dev, planes))
        assert got == [((0, 0, 0, 0), 0)] * len(PAGE_SIZED)
        masks, clean = planes.read()
        assert clean and all(not m.any() for m in masks)
        assert model.ctx.extract_page_boxes_dev(_box_views(dev)[:1]) == [((0, 0, 0, 0), 0)]
    finally:
        model.release()
