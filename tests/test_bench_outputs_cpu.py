"""bench.py --dump-outputs, on CPU: `dump_outputs` writes float32 / float64 .npy files, draws the same seeded sample on every call,
keeps the whole first page only while the 64 MB budget allows, and never exceeds it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _labels(pages, h, w, seed, n_labels=2):
    import torch
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).integers(0, n_labels, (pages, h, w)).astype(np.uint8))


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d)}


def test_dump_is_seeded_typed_and_consistent(tmp_path):
    t = _labels(3, 500, 400, seed=1, n_labels=4)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    assert sorted(bench.dump_outputs(a, {"labels": t})) == sorted(os.listdir(a)) == \
        ["labels_counts.npy", "labels_page0.npy", "labels_sample.npy", "labels_sample_index.npy"]
    bench.dump_outputs(b, {"labels": t})
    da, db = _load(a), _load(b)
    for k in da:
        assert da[k].dtype in (np.float32, np.float64) and np.array_equal(da[k], db[k])
    flat = t.numpy().reshape(-1)
    idx = da["labels_sample_index"].astype(np.int64)
    assert len(idx) == min(bench.DUMP_SAMPLE, flat.size) and np.all(np.diff(idx) >= 0)
    assert np.array_equal(da["labels_sample"], flat[idx].astype(np.float32))
    assert np.array_equal(da["labels_page0"], t[0].numpy().astype(np.float32))
    assert np.array_equal(da["labels_counts"], np.stack([np.bincount(p.reshape(-1), minlength=4) for p in t.numpy()]).astype(np.float64))


def test_dump_stays_inside_the_budget(tmp_path):
    # two outputs whose first pages (2 x 48 MB as float32) cannot both be kept whole: samples and counts of both, one page at most
    big = {"text_regions": _labels(1, 4000, 3000, seed=2)[0], "textlines": _labels(1, 4000, 3000, seed=3)[0]}
    d = str(tmp_path / "big")
    names = bench.dump_outputs(d, big)
    assert sum(os.path.getsize(os.path.join(d, n)) for n in os.listdir(d)) <= bench.DUMP_BUDGET_BYTES
    assert {"text_regions_sample.npy", "textlines_sample.npy", "text_regions_counts.npy", "textlines_counts.npy"} <= set(names)
    assert sum(n.endswith("_page0.npy") for n in names) <= 1
