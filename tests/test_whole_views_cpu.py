"""No GPU: the many-page entry points exist in the library, the header and the binding; the ABI number did not move; and
InferenceStages.run_pages(resident=True) hands foreign model objects to the loop over run(), as the default path does."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sbb_textline_detection_amd import _capi, stages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sbbseg_segment_whole_views_dev", "sbbseg_extract_page_boxes_dev", "sbbseg_run_pages")


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


def test_new_symbols_are_exported_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "sbbseg.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _capi.EXPORTS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert getattr(lib, name).argtypes, name


def test_abi_version_is_still_5(lib):
    assert lib.sbbseg_abi_version() == 5
    assert "#define SBBSEG_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "sbbseg.h")).read()


def test_binding_structs_have_the_header_layout():
    """sbbseg_whole_view: pointer, six ints, pointer; sbbseg_run_page_io: pointer, four ints, three pointers, sbbseg_run_info, int32."""
    p = C.sizeof(C.c_void_p)
    assert _capi.WholeView.labels.offset == p + 6 * 4 and C.sizeof(_capi.WholeView) == 2 * p + 6 * 4
    assert _capi.RunPageIO.page_mask_out.offset == p + 4 * 4
    assert _capi.RunPageIO.info.offset == 4 * p + 4 * 4
    assert _capi.RunPageIO.status.offset == 4 * p + 4 * 4 + C.sizeof(_capi.RunInfo)
    assert C.sizeof(_capi.RunInfo) == 40


def test_null_handle_is_a_status_not_a_crash(lib):
    view = (_capi.WholeView * 1)()
    assert lib.sbbseg_segment_whole_views_dev(None, 1, view) != 0
    assert b"null handle" in lib.sbbseg_last_error()
    assert lib.sbbseg_extract_page_boxes_dev(None, 1, view, None, None) != 0
    io = (_capi.RunPageIO * 1)()
    assert lib.sbbseg_run_pages(None, None, None, 1, io, 3) != 0


def test_resident_run_pages_with_foreign_models_takes_the_loop(monkeypatch):
    class Foreign:                      # not a SegModel: a Keras-like object the reference would hand in
        pass

    class Session:
        def close(self):
            pass

    seen = []

    def fake_run(self, img):
        seen.append(img.shape)
        return (img[:, :, 0] + 1, None, None, [0, img.shape[0], 0, img.shape[1]])

    monkeypatch.setattr(stages, "start_new_session_and_model", lambda path, **kw: (Foreign(), Session()))
    monkeypatch.setattr(stages.InferenceStages, "run", fake_run)
    st = stages.InferenceStages("a.h5", "b.h5", "c.h5")
    images = [np.full((5 + k, 7, 3), k, np.uint8) for k in range(3)]
    want = [st.run(img) for img in images]
    del seen[:]
    for resident in (True, False):
        got = st.run_pages(images, resident=resident)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert np.array_equal(a[0], b[0]) and a[1] is None and a[2] is None and a[3] == b[3]
    assert seen == [img.shape for img in images] * 2
