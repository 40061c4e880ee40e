"""csrc/route.h -- which kernel family runs a plan op -- over every combination of the A/B knobs, without a GPU.

A small host program includes the header, builds a handle by hand (no HIP call; the fragment pointers are dummies that nothing
dereferences) whose plan holds one op of every kind, and prints ``route_of`` of every op and block part for the 256 combinations of
conv variant 0-3 x bits 18, 22, 23, 24, 25 x {f16, f16x3}.  The program is built with the address and undefined-behaviour sanitizers (a
stand-alone host program: nothing is preloaded).

The table it prints is held to ``want_routes`` below: a restatement of the conditions launch_op spelled out op type by op type before
route.h existed (csrc/forward.hip at 19a9b4d) -- each absorbed op RESTATES its absorber's condition there, as that code did, so the
restatement is independent of the header's "ask the absorber" rule."""
import itertools
import os
import shutil
import subprocess

import pytest

ROUTES = ["none", "block_fused", "block_parts", "stem", "stem_pool", "direct64", "c3er", "expand_reduce", "dec_halo", "conv", "pool", "tail",
          "head"]                                 # csrc/route.h enum Route, in order
F16, F16X3 = 2, 3                                 # csrc/internal.h enum Precision

# the plan of the program: op index -> what it is (block parts print as "<op>.<part>")
STEM, POOL, BLOCK, LONE64, C3, EXPAND_A, REDUCE_A, EXPAND_B, REDUCE_B, HALO, PLAIN, TAIL, HEAD = range(13)
OPS = ["0", "1", "2", "2.0", "2.1", "2.2"] + [str(i) for i in range(3, 13)]
ABSORBED = {str(POOL): (str(STEM), {"stem_pool"}), str(C3): (str(EXPAND_A), {"c3er"}),
            str(REDUCE_A): (str(EXPAND_A), {"c3er", "expand_reduce"}), str(REDUCE_B): (str(EXPAND_B), {"expand_reduce"})}

_PROBE = r"""
#include "route.h"
#include <cstdio>
using namespace sbbseg;

static Op conv(const char* name) { Op o{}; o.type = kConv; o.name = name; return o; }

int main()
{
    static uint16_t frag[8];                     // fragment pointers: non-null, never dereferenced
    sbbseg_ctx c;
    std::vector<Op>& ops = c.ops;
    ops.push_back(conv("stem"));      ops.back().conv.d_stem_wfrag = frag; ops.back().conv.fused_pool = 1;
    { Op o{}; o.type = kPool; o.name = "pool"; o.absorbed_by = 0; ops.push_back(o); }
    { Op o{}; o.type = kBlock; o.name = "block";
      o.parts = {conv("block.reduce"), conv("block.3x3"), conv("block.expand")}; o.parts[1].conv.d_d64_wfrag = frag; ops.push_back(o); }
    ops.push_back(conv("lone64"));    ops.back().conv.d_d64_wfrag = frag;
    ops.push_back(conv("c3"));        ops.back().absorbed_by = 5;
    ops.push_back(conv("expand_a"));  ops.back().conv.fused_reduce = 6; ops.back().conv.fused_conv3 = 4;
    ops.push_back(conv("reduce_a"));  ops.back().absorbed_by = 5;
    ops.push_back(conv("expand_b"));  ops.back().conv.fused_reduce = 8;
    ops.push_back(conv("reduce_b"));  ops.back().absorbed_by = 7;
    ops.push_back(conv("halo"));      ops.back().conv.d_halo_wfrag = frag;
    ops.push_back(conv("plain"));
    { Op o{}; o.type = kTail; o.name = "tail"; ops.push_back(o); }
    { Op o{}; o.type = kHead; o.name = "head"; ops.push_back(o); }
    for (int precision : {(int)kF16, (int)kF16X3})
        for (int variant = 0; variant < 4; ++variant)
            for (int bits = 0; bits < 32; ++bits) {
                c.precision = precision; c.conv_variant = variant;
                c.unfuse_blocks = bits & 1; c.unfuse_stem_pool = bits & 2; c.no_dec_halo = bits & 4; c.no_expand_reduce = bits & 8; c.no_c3er = bits & 16;
                printf("%d %d %d", precision, variant, bits);
                for (size_t i = 0; i < ops.size(); ++i) {
                    printf(" %zu=%d", i, (int)route_of(&c, ops[i]));
                    for (size_t k = 0; k < ops[i].parts.size(); ++k) printf(" %zu.%zu=%d", i, k, (int)route_of(&c, ops[i].parts[k]));
                }
                printf("\n");
            }
    return 0;
}
"""


def want_routes(variant, unfuse_blocks, unfuse_stem_pool, no_dec_halo, no_expand_reduce, no_c3er):
    """launch_op's ladder at the parent commit, one op of the program's plan after the other.  Precision is no input: the precision pair
    of a family was chosen inside each branch (and the plan facts -- which fragments and fused_* an op has -- are the program's)."""
    v0 = variant == 0
    r = {}
    # kConv, in the ladder's order: the two early returns, stem (+ pool), direct64, the expand conv (c3er inside), dec_halo, generic
    r[str(STEM)] = ("stem_pool" if not unfuse_stem_pool else "stem") if v0 else "conv"
    r[str(LONE64)] = "direct64" if v0 else "conv"
    r[str(C3)] = "none" if (not no_c3er and not no_expand_reduce and v0) else "conv"               # fused_into_c3 && ...
    for e, red, has_c3 in ((EXPAND_A, REDUCE_A, True), (EXPAND_B, REDUCE_B, False)):
        r[str(red)] = "none" if (not no_expand_reduce and v0) else "conv"                          # fused_into_expand && ...
        if not no_expand_reduce and v0:
            r[str(e)] = "c3er" if (has_c3 and not no_c3er) else "expand_reduce"
        else:
            r[str(e)] = "conv"
    r[str(HALO)] = "dec_halo" if (not no_dec_halo and v0) else "conv"                              # runs_dec_halo
    r[str(PLAIN)] = "conv"
    # kPool: "under exactly the condition that sends the stem there"
    r[str(POOL)] = "none" if (not unfuse_stem_pool and v0) else "pool"
    # kBlock: bit 18 alone; the parts went through launch_op as convs
    r[str(BLOCK)] = "block_parts" if unfuse_blocks else "block_fused"
    r["%d.0" % BLOCK] = r["%d.2" % BLOCK] = "conv"
    r["%d.1" % BLOCK] = "direct64" if v0 else "conv"
    r[str(TAIL)], r[str(HEAD)] = "tail", "head"
    return r


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("route")
    (d / "probe.cpp").write_text(_PROBE)
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbb_textline_detection_amd", "csrc")
    # route.h is host only: it must compile without the device pass and run without the HIP runtime being called
    res = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                          "-Xarch_host", "-fno-sanitize-recover=all", "-I", csrc, str(d / "probe.cpp"), "-o", str(d / "probe")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    out = subprocess.run([str(d / "probe")], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stderr[-3000:]              # (a sanitizer report ends the program with a status)
    rows = {}
    for line in out.stdout.splitlines():
        f = line.split()
        rows[tuple(int(x) for x in f[:3])] = {k: ROUTES[int(v)] for k, v in (kv.split("=") for kv in f[3:])}
    return rows


def test_header_is_host_only():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbb_textline_detection_amd", "csrc")
    text = open(os.path.join(csrc, "route.h")).read()
    import re
    assert re.findall(r'#\s*include\s+"([^"]+)"', text) == ["ctx.h"]
    for word in ("HIPCHK", "REQUIRE", "hipMemcpy", "hipMalloc", "hipLaunch", "<<<"):
        assert word not in text, word


def test_the_sweep_is_complete(table):
    assert sorted(table) == sorted(itertools.product((F16, F16X3), range(4), range(32))) and len(table) == 256
    assert all(sorted(row) == sorted(OPS) for row in table.values())


def test_routes_match_the_parent_ladder(table):
    bad = []
    for (precision, variant, bits), got in sorted(table.items()):
        want = want_routes(variant, bits & 1, bits & 2, bits & 4, bits & 8, bits & 16)
        bad += [(precision, variant, bits, op, got[op], want[op]) for op in OPS if got[op] != want[op]]
    assert not bad, (len(bad), bad[:8])


def test_what_the_table_pins(table):
    """the two properties of the parent's ladder that nothing else states: the fused block does not look at the tile-family variants, and
    variants 1-3 send the stem and the 64 -> 64 3x3 conv to the generic kernel"""
    for (precision, variant, bits), got in table.items():
        assert got[str(BLOCK)] == ("block_parts" if bits & 1 else "block_fused")
        if variant:
            assert got[str(STEM)] == got[str(LONE64)] == got["%d.1" % BLOCK] == "conv" and got[str(POOL)] == "pool"
            assert "none" not in got.values()
    assert table[(F16X3, 0, 0)] == table[(F16, 0, 0)] and [table[(F16X3, 0, 0)][o] for o in OPS] == [
        "stem_pool", "none", "block_fused", "conv", "direct64", "conv", "direct64", "none", "c3er", "none", "expand_reduce", "none", "dec_halo",
        "conv", "tail", "head"]


def test_absorbed_ops_agree_with_their_absorbers(table):
    """an absorbed op launches nothing if and only if its absorber takes a route that writes it -- so no op is computed twice or never --
    and nothing else launches nothing"""
    for key, got in table.items():
        for op, (absorber, writing) in ABSORBED.items():
            assert (got[op] == "none") == (got[absorber] in writing), (key, op, got[op], absorber, got[absorber])
        assert {op for op in OPS if got[op] == "none"} <= set(ABSORBED), key
        # the writing routes are taken by absorbers only, and each writes ops that exist in the plan
        assert {op for op in OPS if got[op] in ("stem_pool", "c3er", "expand_reduce")} <= {a for a, _ in ABSORBED.values()}, key
