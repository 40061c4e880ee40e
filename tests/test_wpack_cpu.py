"""csrc/wpack.h -- the host-only weight packer behind plan building -- against tests/wpack_ref.py, bit for bit, without a GPU.

A small host program includes the header, fills fp32 weights from the integer recurrence the restatement uses too, and writes what
the packer returns; the cases are the kernels' own fixed shapes.  The program is built with the address and undefined-behaviour
sanitizers (a stand-alone host program: nothing is preloaded), so an index that leaves a fragment or a matrix fails the test too."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import wpack_ref as ref

PRECISIONS = {ref.BF16: 0, ref.F32: 1, ref.F16: 2, ref.F16X3: 3}              # csrc/internal.h enum Precision
HALF_MODES = [ref.F16, ref.BF16, ref.F16X3]
VARIANTS = ["rand", "zero", "tiny", "big"]

_PROBE = r"""
#include "wpack.h"
#include <cstdio>
#include <cstdlib>
#include <string>
using namespace sbbseg;

static uint32_t lcg_state;
static uint32_t lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return lcg_state; }

static std::vector<float> weights(size_t n, uint32_t seed, const std::string& variant)
{
    lcg_state = seed;
    std::vector<float> w(n);
    for (size_t i = 0; i < n; ++i) w[i] = (float)((int)((lcg() >> 8) % 65535u) - 32767) / 32768.f;
    if (variant == "zero") for (float& v : w) v = 0.f;
    else if (variant == "tiny") { for (float& v : w) v = std::ldexp(v, -71); w[0] = std::ldexp(1.f, -70); }
    else if (variant == "big") w[1] = 70000.f;
    else { w[2] = (300.f + std::ldexp(1.f, -15)) / 512.f; w[3] = 0.75f; }
    return w;
}
static std::vector<uint16_t> halves(size_t n, uint32_t seed)
{
    lcg_state = seed;
    std::vector<uint16_t> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = (uint16_t)((lcg() >> 8) & 0xffffu);
    return h;
}
template <class T> static void put(const std::vector<T>& v)
{
    const uint64_t bytes = v.size() * sizeof(T);
    fwrite(&bytes, sizeof(bytes), 1, stdout);
    fwrite(v.data(), 1, bytes, stdout);
}
static float wpre_of(int precision, const std::vector<float>& a, const std::vector<float>* b = nullptr)
{
    if (!is_split(precision)) return 1.f;
    return split_prescale(max_abs(a.data(), a.size(), b ? max_abs(b->data(), b->size()) : 0.f));
}
static sbbseg_conv_src src(int tensor, int channels, int kh, int kw, int stride, int pad, int off)
{
    return {tensor, channels, kh, kw, stride, stride, pad, pad, 0, off, off};
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const std::string what = argv[1], variant = argv[3];
    const int precision = atoi(argv[2]);
    std::vector<uint16_t> out;
    if (what == "stem") {                        // the call of each case = its call in plan_build.hip
        const auto w = weights(7 * 4 * 8 * 64, 1, variant);
        weight_frags(out, precision, wpre_of(precision, w), w.data(), 7 * 32, 64, false);
        put(out);
    } else if (what == "direct64") {
        const auto w = weights(9 * 64 * 64, 2, variant);
        weight_frags(out, precision, wpre_of(precision, w), w.data(), 9 * 64, 64, false);
        put(out);
    } else if (what == "w1_64" || what == "w1_256") {
        const int cin = what == "w1_64" ? 64 : 256;
        const auto w = weights((size_t)cin * 64, 3, variant);
        weight_frags(out, precision, wpre_of(precision, w), w.data(), cin, 64, true);
        put(out);
    } else if (what == "w3_id" || what == "w3_ab" || what == "w3_ba") {
        const auto a = weights(64 * 256, 4, variant), b = weights(64 * 256, 5, "rand");
        const float wpre = wpre_of(precision, a, what == "w3_id" ? nullptr : &b);
        weight_frags(out, precision, wpre, (what == "w3_ba" ? b : a).data(), 64, 256, true);
        if (what != "w3_id") weight_frags(out, precision, wpre, (what == "w3_ba" ? a : b).data(), 64, 256, true);
        put(out);
    } else if (what == "tail") {
        const auto w0 = weights(9 * 64 * 32, 6, variant), wi = weights(9 * 3 * 32, 7, variant);
        const auto pre = tail_presum(is_split(precision), w0.data(), wi.data());
        const int KS = is_split(precision) ? kTailSplitKSteps : kTailKSteps;
        for (int q = 0; q < 4; ++q) weight_frags(out, precision, wpre_of(precision, pre), &pre[(size_t)q * KS * 64 * 32], KS * 64, 32, false);
        put(out);
    } else if (what == "relay") {
        const auto m64 = halves((size_t)64 * 26 * 64, 8), m128 = halves((size_t)128 * 36 * 64, 9);
        matrix_frags(out, m64.data(), 26 * 64, 0, 4, 26);                                   // dec_halo, one class
        put(out);
        out.clear();
        matrix_frags(out, m128.data(), 36 * 64, 0, 128 / 16, 36);                            // conv3
        put(out);
        out.clear();
        const auto m3 = halves((size_t)512 * 256, 10), m1 = halves((size_t)128 * 1024, 11);
        for (int j = 0; j < 128 / 64; ++j) matrix_frags(out, m3.data(), 256, j * 16, 16, 128 / 32);      // expand
        put(out);
        out.clear();
        matrix_frags(out, m1.data(), 1024, 0, 128 / 16, 4 * 128 / 32);                       // reduce
        put(out);
    } else if (what == "conv_a" || what == "conv_b" || what == "conv_c") {
        sbbseg_conv_desc d = {};
        int src_C[2] = {0, 0};
        d.n_src = 1;
        if (what == "conv_a") { d.src[0] = src(0, 64, 1, 1, 1, 0, 0); src_C[0] = 64; d.cout = 64; }
        else if (what == "conv_b") { d.src[0] = src(0, 24, 3, 3, 1, 1, 0); src_C[0] = 24; d.cout = 8; }
        else { d.n_src = 2; d.src[0] = src(0, 32, 2, 2, 1, 1, 0); d.src[1] = src(1, 64, 3, 3, 2, 1, 1); src_C[0] = 32; src_C[1] = 64; d.cout = 16; }
        const auto w0 = weights((size_t)d.src[0].kh * d.src[0].kw * d.src[0].channels * d.cout, 12, variant);
        const auto w1 = weights(d.n_src == 2 ? (size_t)d.src[1].kh * d.src[1].kw * d.src[1].channels * d.cout : 4, 13, "rand");
        const ConvKTable kt = conv_ktable(d, src_C, precision, true);
        std::vector<int32_t> ktab, ksteps, meta = {kt.ksteps_src[0], kt.ksteps_src[1], kt.total_ksteps};
        for (const KTabEntry& e : kt.ktab) { ktab.push_back(e.dy); ktab.push_back(e.dx); ktab.push_back(e.coff); }
        for (const KStepRec& r : kt.ksteps) { ksteps.push_back(r.dy); ksteps.push_back(r.dx); ksteps.push_back(r.coff); ksteps.push_back(r.irregular); }
        for (int s = 0; s < 2; ++s) for (int a = 0; a < 2; ++a) meta.push_back(kt.tap_lo[s][a]);
        for (int s = 0; s < 2; ++s) for (int a = 0; a < 2; ++a) meta.push_back(kt.tap_hi[s][a]);
        meta.push_back(kt.fg_ok ? 1 : 0);
        put(ktab); put(ksteps); put(meta);
        const float* const ws[2] = {w0.data(), w1.data()};
        const int bc = precision != kF32 ? 256 : 4, cout_pad = (d.cout + bc - 1) / bc * bc;
        const float wpre = wpre_of(precision, w0, d.n_src == 2 ? &w1 : nullptr);
        if (precision == kF32) put(conv_pack_matrix<float>(kt, d, ws, precision, cout_pad, wpre));
        else put(conv_pack_matrix<uint16_t>(kt, d, ws, precision, cout_pad, wpre));
    } else {
        return 2;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("wpack")
    (d / "probe.cpp").write_text(_PROBE)
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbb_textline_detection_amd", "csrc")
    # wpack.h is host only: it must compile without the device pass and link without the HIP runtime being called
    res = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc, str(d / "probe.cpp"), "-o", str(d / "probe")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]

    def run(what, precision, variant="rand"):
        out = subprocess.run([str(d / "probe"), what, str(PRECISIONS[precision]), variant], capture_output=True)
        assert out.returncode == 0, out.stderr.decode()[-3000:]
        buf, sections = out.stdout, []
        while buf:
            n = int(np.frombuffer(buf[:8], np.uint64)[0])
            sections.append(buf[8:8 + n])
            buf = buf[8 + n:]
        return sections
    return run


def _same(got, want, what):
    got = np.frombuffer(got, want.dtype)
    assert got.shape == want.ravel().shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want.ravel())
    assert bad.size == 0, (what, bad.size, bad[:8], got[bad[:8]], want.ravel()[bad[:8]])


def test_header_is_host_only_and_stands_alone():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbb_textline_detection_amd", "csrc")
    text = open(os.path.join(csrc, "wpack.h")).read()
    import re
    assert re.findall(r'#\s*include\s+"([^"]+)"', text) == ["internal.h"]
    for word in ("sbbseg_ctx", "upload(", "REQUIRE", "hipMemcpy", "hipMalloc"):
        assert word not in text, word


def test_roundings_of_the_restatement():
    """the restatement's own roundings on figures worked out by hand"""
    assert ref.f16_bits(np.float32([70000, -70000, 65520, 1, 2.0 ** -24, 2.0 ** -25])).tolist() == [0x7BFF, 0xFBFF, 0x7BFF, 0x3C00, 1, 0]
    assert ref.bf16_bits(np.float32([1, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8])).tolist() == [0x3F80, 0x3F80, 0x3F82]        # ties to even
    assert ref.prescale(0) == 1 and ref.prescale(1) == 256 and ref.prescale(0.75) == 512 and ref.prescale(511) == 1 and ref.prescale(512) == 0.5
    assert ref.prescale(2.0 ** -70) == 2.0 ** 60 and ref.prescale(3e38) == 2.0 ** -60
    hi, lo = ref.split_bits(np.float32([(300 + 2.0 ** -15) / 512]), 512)
    assert hi.view(np.float16)[0] == 300 and lo[0] == 0x0200                      # 2^-15 = 512 x 2^-24: a subnormal half
    assert ref.row_channel(np.arange(16), 64).tolist() == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27]
    assert sorted(ref.row_channel(np.arange(256), 256).tolist()) == list(range(256)) and ref.row_channel(16, 64) == 4 and ref.row_channel(40, 32) == 48


def _w(shape, seed, variant):
    return ref.weights(int(np.prod(shape)), seed, variant).reshape(shape)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("precision", HALF_MODES)
def test_fragments_from_fp32_weights(probe, precision, variant):
    _same(probe("stem", precision, variant)[0], ref.stem(precision, _w((7, 4, 8, 64), 1, variant)), "stem")
    _same(probe("direct64", precision, variant)[0], ref.direct64(precision, _w((9, 64, 64), 2, variant)), "direct64")
    for cin in (64, 256):
        _same(probe("w1_%d" % cin, precision, variant)[0], ref.block_w1(precision, _w((cin, 64), 3, variant)), "w1 %d" % cin)
    a, b = _w((64, 256), 4, variant), _w((64, 256), 5, "rand")
    _same(probe("w3_id", precision, variant)[0], ref.block_w3(precision, a), "w3 identity")
    _same(probe("w3_ab", precision, variant)[0], ref.block_w3(precision, a, b), "w3 [b, x]")
    _same(probe("w3_ba", precision, variant)[0], ref.block_w3(precision, b, a), "w3 [x, b]")
    got = probe("tail", precision, variant)[0]
    assert len(got) == 2 * 4 * (5 * 2 if precision == ref.F16X3 else 6) * 4 * 512
    _same(got, ref.tail(precision, _w((3, 3, 64, 32), 6, variant), _w((3, 3, 3, 32), 7, variant)), "tail")


def test_the_variants_reach_the_prescale_edges(probe):
    """what the weight variants are there for, seen in the packer's own output"""
    stem = {v: np.frombuffer(probe("stem", ref.F16X3, v)[0], np.uint16) for v in VARIANTS}
    assert not stem["zero"].any()
    lo = stem["rand"][stem["rand"].size // 2:]
    assert ((lo & 0x7C00) == 0).any() and (lo[(lo & 0x7C00) == 0] & 0x3FF).any()                 # a subnormal lo half
    assert stem["tiny"].view(np.float16).max() == np.float16(2.0 ** -10)                         # 2^-70 x 2^60: the clamp, not [256, 512)
    assert stem["big"].view(np.float16).max() == np.float16(70000 / 256)                         # pre-scaled down, nothing saturates
    assert (np.frombuffer(probe("stem", ref.F16, "big")[0], np.uint16) & 0x7FFF).max() == 0x7BFF   # plain fp16: 65504, no infinity


def test_fragments_from_packed_matrices(probe):
    halo, c3, ex, rd = probe("relay", ref.F16X3)
    _same(halo, ref.dec_halo(ref.halves(64 * 26 * 64, 8).reshape(64, -1), 26), "dec_halo")
    _same(c3, ref.conv3(ref.halves(128 * 36 * 64, 9).reshape(128, -1), 128, 36), "conv3")
    _same(ex, ref.expand(ref.halves(512 * 256, 10).reshape(512, -1), 128, 32), "expand")
    _same(rd, ref.reduce(ref.halves(128 * 1024, 11).reshape(128, -1), 128, 32), "reduce")


CONVS = {       # name -> (sources, cout): a pointwise conv; channel padding and irregular steps; two sources, the grouped tap order, an offset
    "conv_a": ([ref.Src(64, 64, 1, 1)], 64),
    "conv_b": ([ref.Src(24, 24, 3, 3, pad=1)], 8),
    "conv_c": ([ref.Src(32, 32, 2, 2, pad=1), ref.Src(64, 64, 3, 3, stride=2, pad=1, off=1)], 16),
}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("precision", HALF_MODES + [ref.F32])
@pytest.mark.parametrize("name", sorted(CONVS))
def test_conv_tables_and_packed_matrix(probe, name, precision, variant):
    srcs, cout = CONVS[name]
    ws = [_w((s.kh, s.kw, s.channels, cout), 12 + i, variant if i == 0 else "rand") for i, s in enumerate(srcs)]
    slots, ktab, ksteps, per_src = ref.conv_tables(precision, srcs)
    got_ktab, got_ksteps, got_meta, got_mat = probe(name, precision, variant)
    _same(got_ktab, np.array(ktab, np.int32), "ktab")
    _same(got_ksteps, np.array(ksteps, np.int32), "ksteps")
    _same(got_meta, np.array(ref.conv_meta(ksteps, per_src), np.int32), "meta")
    want = ref.conv_matrix(precision, srcs, cout, ws, slots)
    _same(got_mat, want.view(np.uint32) if precision == ref.F32 else want, "matrix")


def test_conv_cases_reach_both_kinds_of_k_step():
    kinds = {(name, p): [k[3] for k in ref.conv_tables(p, CONVS[name][0])[2]] for name in CONVS for p in HALF_MODES}
    assert not any(kinds[("conv_a", ref.F16)]) and len(kinds[("conv_a", ref.F16)]) == 1 and len(kinds[("conv_a", ref.F16X3)]) == 2
    assert all(kinds[("conv_b", ref.F16)]) and len(kinds[("conv_b", ref.F16)]) == 4                       # 27 granules: 5 slots of padding
    assert kinds[("conv_c", ref.F16X3)] == [0] * 22 and any(kinds[("conv_b", ref.F16X3)]) and kinds[("conv_c", ref.F16)] == [1, 1] + [0] * 9
    taps = [k[:2] for k in ref.conv_tables(ref.F16, CONVS["conv_c"][0])[2][2:]]
    assert taps == [(ky - 2, kx - 2) for ky, kx in [(0, 0), (0, 2), (2, 0), (2, 2), (0, 1), (2, 1), (1, 0), (1, 2), (1, 1)]]
