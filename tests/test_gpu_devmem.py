"""-m gpu: a handle's device memory belongs to one registry (csrc/devmem.h).  What ``sbbseg_device_bytes`` reports follows every allocation and
release exactly, grow-only buffers grow once per size, a plan call that fails gives back what it uploaded, and ``sbbseg_destroy`` succeeds
after every buffer family has been used.  The net is ``convT_k2`` of tests/small_plans.py (64 x 96 input, three classes): its
Conv2DTranspose decoder is lowered to parity classes, which plan building merges into one op (releasing the absorbed classes' constants)."""
import ctypes as C

import numpy as np
import pytest

from sbb_textline_detection_amd import _capi
from sbb_textline_detection_amd.model import SegModel
from sbb_textline_detection_amd.synthetic import synthetic_page

from small_plans import small_net

pytestmark = pytest.mark.gpu
PRECISIONS = ("f16", "f16x3")
SMALL, LARGE = (64, 96), (150, 200)                     # one tile; 3 x 3 tiles of the 64 x 96 input


def _model(precision):
    cfg, w, _ = small_net("convT_k2")
    return SegModel(cfg, w, device=0, max_batch=4, precision=precision)


@pytest.fixture(scope="module")
def pages():
    return synthetic_page(*SMALL, seed=1), synthetic_page(*LARGE, seed=2)


@pytest.fixture(scope="module", params=PRECISIONS)
def model(request):
    m = _model(request.param)
    assert any("_par4" in op["name"] for op in m.ctx.ops()), [op["name"] for op in m.ctx.ops()]      # the parity merge happened
    yield m
    m.release()


def test_device_alloc_and_free_move_device_bytes_exactly(model):
    ctx = model.ctx
    base = ctx.device_bytes()
    assert base > 0
    sizes = (1, 4096, 100003)
    ptrs = []
    for k, n in enumerate(sizes):
        ptrs.append(ctx.device_alloc(n))
        assert ctx.device_bytes() == base + sum(sizes[:k + 1])
    lib = ctx.lib
    # not the handle's to free: an address inside a handed-out block, and one past it; nothing moves
    for bad in (ptrs[1] + 16, ptrs[2] + sizes[2]):
        assert lib.sbbseg_device_free(ctx.h, C.c_void_p(bad)) != 0 and b"not allocated by this handle" in lib.sbbseg_last_error()
        assert ctx.device_bytes() == base + sum(sizes)
    ctx.device_free(ptrs[1])                                                   # the middle one first
    assert ctx.device_bytes() == base + sizes[0] + sizes[2]
    assert lib.sbbseg_device_free(ctx.h, C.c_void_p(ptrs[1])) != 0             # (twice is refused too)
    ctx.device_free(ptrs[0])
    ctx.device_free(ptrs[2])
    assert ctx.device_bytes() == base
    assert lib.sbbseg_device_free(ctx.h, None) == 0


def test_device_free_refuses_the_handles_own_blocks(model, pages):
    """sbbseg_run_pages leaves its planes in buffers of the layout handle (sbbseg_run_pages_planes names them): blocks of the registry, but
    not handed out by sbbseg_device_alloc, so not the caller's to free."""
    ctx = model.ctx
    h, w = LARGE
    out = _capi.run_pages(ctx, ctx, ctx, [(pages[1], h, w)], channels=1)
    regions, textlines = _capi.run_pages_planes(ctx)
    own = [p for p, _, _ in regions + textlines if p]
    assert out[0][4] == 0 and own, (out[0][3].box_xywh[:], out[0][4])
    before = ctx.device_bytes()
    for p in own:
        assert ctx.lib.sbbseg_device_free(ctx.h, C.c_void_p(p)) != 0 and b"not allocated by this handle" in ctx.lib.sbbseg_last_error()
    assert ctx.device_bytes() == before
    assert np.array_equal(ctx.download(own[0], (8,)), ctx.download(own[0], (8,)))      # (still there)


def test_page_buffers_grow_once_per_size(model, pages):
    small, large = pages
    first = model.segment_page(small)
    b1 = model.ctx.device_bytes()
    assert np.array_equal(model.segment_page(small), first) and model.ctx.device_bytes() == b1
    big = model.segment_page(large)
    b2 = model.ctx.device_bytes()
    assert big.shape == LARGE and b2 > b1
    assert np.array_equal(model.segment_page(large), big) and model.ctx.device_bytes() == b2
    last = model.segment_page(small)
    assert model.ctx.device_bytes() == b2
    assert np.array_equal(last, first)


def test_failed_add_conv_gives_back_what_it_uploaded(model, pages):
    """sbbseg_add_conv uploads the conv's weights, tables and scale / shift before it checks raw_scale / raw_shift: the failing call (an
    argument error: a status, no fault) must leave sbbseg_device_bytes where it was, and the handle must destroy cleanly."""
    before = model.segment_page(pages[0])
    lib = _capi.load_library()
    h = C.c_void_p()
    assert lib.sbbseg_create(0, _capi.PRECISIONS[model.precision], C.byref(h)) == 0
    try:
        t = [C.c_int(-1) for _ in range(3)]
        assert lib.sbbseg_set_input(h, 64, 96, 3) == 0
        assert lib.sbbseg_input_form(h, _capi.INPUT_C8, 0, C.byref(t[0])) == 0
        assert lib.sbbseg_add_tensor(h, 64, 96, 8, C.byref(t[1])) == 0 and lib.sbbseg_add_tensor(h, 64, 96, 8, C.byref(t[2])) == 0
        rng = np.random.RandomState(0)
        wts = rng.randn(3, 3, 3, 8).astype(np.float32)
        scale, shift = np.ones(8, np.float32), np.zeros(8, np.float32)
        d = _capi.ConvDesc()
        d.n_src = 1
        d.src[0] = _capi.ConvSrc(t[0].value, 3, 3, 3, 1, 1, 1, 1, 0, 0, 0)
        d.cout, d.out_h, d.out_w = 8, 64, 96
        d.out_stride_y = d.out_stride_x = 1
        d.out_tensor, d.relu, d.residual_tensor, d.raw_out_tensor, d.head_classes = t[1].value, 1, -1, -1, 0
        size = C.c_size_t()

        def device_bytes():
            assert lib.sbbseg_device_bytes(h, C.byref(size)) == 0
            return size.value

        args = (_capi._ptr(wts), None, _capi._ptr(scale), _capi._ptr(shift))
        assert lib.sbbseg_add_conv(h, C.byref(d), *args, None, None, None, None, None) == 0, lib.sbbseg_last_error()
        held = device_bytes()
        assert held >= wts.nbytes // 2
        d.raw_out_tensor = t[2].value                                          # ... and no raw_scale / raw_shift
        assert lib.sbbseg_add_conv(h, C.byref(d), *args, None, None, None, None, None) != 0
        assert b"raw output needs raw_scale/raw_shift" in lib.sbbseg_last_error()
        assert device_bytes() == held
        n = C.c_int()
        assert lib.sbbseg_num_ops(h, C.byref(n)) == 0 and n.value == 1
        assert lib.sbbseg_add_conv(h, C.byref(d), *args, _capi._ptr(scale), _capi._ptr(shift), None, None, None) == 0      # (the handle serves on)
        assert device_bytes() > held
    finally:
        rc = lib.sbbseg_destroy(h)
    assert rc == 0
    again = _model(model.precision)
    try:
        assert np.array_equal(again.segment_page(pages[0]), before)
    finally:
        again.release()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_buffer_family_once_then_destroy(precision, pages):
    small, large = pages
    m = _model(precision)
    ctx = m.ctx
    try:
        views = ctx.segment_views([(small, *SMALL, (0, 0, SMALL[1], SMALL[0]), False), (large, *LARGE, (0, 0, LARGE[1], LARGE[0]), True)])
        assert views[0][0].shape == SMALL and views[1][0].shape == LARGE
        assert ctx.segment_whole(large, *LARGE).shape == LARGE
        rng = np.random.RandomState(5)
        plane = (rng.rand(*LARGE) < 0.97).astype(np.uint8)
        plane[:, 95:105] = 0                                                   # two regions, left and right
        assert ctx.morph(plane, 0, 5, 2).shape == LARGE
        boxes = ctx.text_region_boxes(plane)
        assert len(boxes) >= 1
        two = [[0, 0, 95, 150], [105, 0, 95, 150]]
        slopes = ctx.region_deskew_slopes(plane, two)
        assert len(slopes) == 2
        assert len(ctx.region_line_boxes(plane, two, slopes)) == 2
        got = ctx.segment_pages([large, large[::-1].copy()])
        assert len(got) == 2 and np.array_equal(got[0], ctx.segment_page(large))
        assert ctx.device_bytes() > 0
    finally:
        rc = ctx.lib.sbbseg_destroy(ctx.h)
        ctx.h = None
    assert rc == 0
