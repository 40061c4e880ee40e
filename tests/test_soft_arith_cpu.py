"""csrc/profile_stat.h's soft_div and soft_sqrt alone, without a GPU and without the library: they claim IEEE-754 binary64 round to nearest
even for every class of operand, and the deskew statistic's bit-for-bit agreement with numpy rests on that.

A small host program includes only that header, reads operand bit patterns from a binary file and prints the result bits.  It is built with
the address and undefined-behaviour sanitizers (a stand-alone host program: nothing is preloaded; the shifts by computed amounts are what
could go wrong).  What it prints is held to numpy's ``/`` and ``np.sqrt`` bit for bit; a NaN must be the canonical quiet NaN."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

import profile_cases as pc

_PROBE = r"""
#include "profile_stat.h"
#include <cstdio>
#include <vector>
using namespace sbbseg;

// file: int64 op, int64 n, n doubles a, (op 0) n doubles b
int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    long long head[2];
    while (fread(head, sizeof(long long), 2, f) == 2) {
        const long long op = head[0], n = head[1];
        if ((op != 0 && op != 1) || n < 0) return 3;
        std::vector<double> a((size_t)n), b((size_t)n);
        if (fread(a.data(), sizeof(double), (size_t)n, f) != (size_t)n) return 3;
        if (op == 0 && fread(b.data(), sizeof(double), (size_t)n, f) != (size_t)n) return 3;
        for (long long i = 0; i < n; ++i) printf("%016llx\n", (unsigned long long)f64_bits(op == 0 ? soft_div(a[i], b[i]) : soft_sqrt(a[i])));
    }
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def cases():
    div, sqrt = pc.soft_arith_operands()
    return div, sqrt, pc.numpy_results(div, sqrt)


@pytest.fixture(scope="module")
def printed(tmp_path_factory, cases):
    """{("div" | "sqrt", family): result bits as float64}"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    div, sqrt, _want = cases
    d = tmp_path_factory.mktemp("soft_arith")
    (d / "probe.cpp").write_text(_PROBE)
    with open(d / "operands.bin", "wb") as f:
        for a, b in div.values():
            f.write(np.array([0, a.size], np.int64).tobytes() + np.ascontiguousarray(a).tobytes() + np.ascontiguousarray(b).tobytes())
        for a in sqrt.values():
            f.write(np.array([1, a.size], np.int64).tobytes() + np.ascontiguousarray(a).tobytes())
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbb_textline_detection_amd", "csrc")
    # profile_stat.h is plain C++ for the host: it compiles without the HIP language and without the HIP runtime's headers
    res = subprocess.run([hipcc, "-x", "c++", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc, str(d / "probe.cpp"), "-o", str(d / "probe")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    t = time.time()
    out = subprocess.run([str(d / "probe"), str(d / "operands.bin")], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-3000:]              # (a sanitizer report ends the program with a status)
    got = np.array([int(v, 16) for v in out.stdout.split()], np.uint64).view(np.float64)
    print(f"[test_soft_arith_cpu] {got.size} operand sets, sanitized host program {time.time() - t:.2f} s")
    res, at = {}, 0
    for op, families in (("div", div), ("sqrt", sqrt)):
        for name, v in families.items():
            n = (v[0] if op == "div" else v).size
            res[(op, name)] = got[at:at + n]
            at += n
    assert at == got.size
    return res


def test_operand_families_hold_what_they_promise(cases):
    div, sqrt, (want_div, want_sqrt) = cases
    total = sum(a.size for a, _b in div.values()) + sum(a.size for a in sqrt.values())
    assert 200000 <= total <= 900000, total
    tiny, big = np.finfo(np.float64).tiny, np.finfo(np.float64).max
    q = np.abs(want_div["subnormal quotients"])
    assert ((q > 0) & (q < tiny)).sum() > 10000 and (q == 0).sum() > 100 and (q >= tiny).sum() > 100
    q = np.abs(want_div["overflowing quotients"])
    assert np.isinf(q).sum() > 1000 and (q <= big).sum() > 1000
    sp = want_div["specials"]
    assert np.isnan(sp).any() and np.isinf(sp).any() and (sp == 0).any() and ((np.abs(sp) > 0) & (np.abs(sp) < tiny)).any()
    r = want_sqrt["squares"]
    assert np.array_equal(r * r, sqrt["squares"]) and r.max() == 2.0 ** 26
    assert np.isnan(want_sqrt["specials"]).sum() >= sqrt["specials"].size // 2 - 2      # every negative but -0
    assert (sqrt["subnormals"] < tiny).all() and (sqrt["subnormals"] > 0).all()
    e = (pc.bits(sqrt["even and odd exponents"]) >> np.uint64(52)) & np.uint64(1)
    assert (e == 0).sum() > 5000 and (e == 1).sum() > 5000


def test_soft_div_is_numpys_divide_in_every_bit(cases, printed):
    div, _sqrt, (want, _w) = cases
    for name in div:
        got = printed[("div", name)]
        assert got.shape == want[name].shape and pc.soft_arith_mismatches(got, want[name]) == 0, name


def test_soft_sqrt_is_numpys_sqrt_in_every_bit(cases, printed):
    _div, sqrt, (_w, want) = cases
    for name in sqrt:
        got = printed[("sqrt", name)]
        assert got.shape == want[name].shape and pc.soft_arith_mismatches(got, want[name]) == 0, name
