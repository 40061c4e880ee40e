"""csrc/devmem.h -- the registry that owns a handle's device and pinned memory, its grow-only buffers and scope guards -- without a GPU.

A small host program includes the header (which includes no HIP header) and drives a DeviceMem whose backend is malloc / free plus counters.
It is built with the address and undefined-behaviour sanitizers and run directly (a stand-alone host program: nothing is preloaded), so the
leak checker reports any block release_all() misses and the address checker any block freed twice.  Each section of the program prints
``PASS <section>`` when all of its checks held, and ``FAIL <line>: <expression>`` for each that did not."""
import os
import shutil
import subprocess

import pytest

SECTIONS = ("bytes_follow_live_blocks", "release", "ensure", "mark_and_release_since", "release_all_and_user_flag", "scope_guards")

_PROBE = r"""
#include "devmem.h"
#include <cstdio>
#include <cstdlib>
#include <set>
using namespace sbbseg;

static int n_alloc = 0, n_free = 0, fail_next = 0, section_fails = 0;
static std::set<void*> live;                           // what the backend has handed out and not got back
static std::vector<void*> freed;                       // in order
static int b_alloc(void** p, size_t bytes)
{
    ++n_alloc;
    if (fail_next) { --fail_next; return 1; }
    *p = bytes ? malloc(bytes) : nullptr;
    if (*p) live.insert(*p);
    return 0;
}
static int b_free(void* p)
{
    ++n_free;
    if (!live.erase(p)) { printf("FAIL backend: free of %p, which is not live\n", p); ++section_fails; return 1; }
    freed.push_back(p);
    free(p);
    return 0;
}
#define CHECK(x) do { if (!(x)) { printf("FAIL %d: %s\n", __LINE__, #x); ++section_fails; } } while (0)
static void section(const char* name) { if (!section_fails) printf("PASS %s\n", name); section_fails = 0; }
static size_t live_sum(const DeviceMem& m) { size_t s = 0; for (const auto& b : m.blocks()) s += b.bytes; return s; }

int main()
{
    {   // bytes() is the sum of the live blocks after every step of a scripted sequence
        DeviceMem m(b_alloc, b_free);
        const size_t sizes[6] = {16, 1, 4096, 33, 7, 100000};
        void* p[6] = {};
        size_t want = 0;
        CHECK(m.bytes() == 0);
        for (int i = 0; i < 6; ++i) {
            CHECK(m.alloc(&p[i], sizes[i]) == 0 && p[i]);
            want += sizes[i];
            CHECK(m.bytes() == want && live_sum(m) == want && m.blocks().size() == (size_t)i + 1);
        }
        const int order[6] = {3, 0, 5, 1, 4, 2};
        for (int k = 0; k < 6; ++k) {
            CHECK(m.release(p[order[k]]) == 0);
            want -= sizes[order[k]];
            CHECK(m.bytes() == want && live_sum(m) == want && live.size() == m.blocks().size());
            if (k == 2) { void* q = nullptr; CHECK(m.alloc(&q, 50) == 0); want += 50; CHECK(m.bytes() == want); CHECK(m.release(q) == 0); want -= 50; }
        }
        CHECK(m.bytes() == 0 && live.empty());
        void* z = (void*)0x10;                          // a zero-byte request: a null pointer, nothing to own
        CHECK(m.alloc(&z, 0) == 0 && z == nullptr && m.blocks().empty() && m.bytes() == 0);
        fail_next = 1;                                  // a failed request leaves the pointer and the total alone
        void* keep = (void*)0x20;
        CHECK(m.alloc(&keep, 64) != 0 && keep == (void*)0x20 && m.bytes() == 0 && m.blocks().empty());
    }
    section("bytes_follow_live_blocks");
    {
        DeviceMem m(b_alloc, b_free);
        void *a = nullptr, *b = nullptr, *c = nullptr;
        CHECK(!m.alloc(&a, 10) && !m.alloc(&b, 20) && !m.alloc(&c, 30));
        int f0 = n_free; freed.clear();
        CHECK(m.release(b) == 0);                       // a middle block: exactly that block
        CHECK(n_free == f0 + 1 && freed.size() == 1 && freed[0] == b && m.bytes() == 40 && m.find(a) && m.find(c) && !m.find(b));
        f0 = n_free;
        CHECK(m.release(nullptr) == 0 && n_free == f0 && m.bytes() == 40);
        int foreign = 0;
        CHECK(m.release(&foreign) != 0 && n_free == f0 && m.bytes() == 40 && m.blocks().size() == 2);      // an error that frees nothing
        CHECK(m.release((char*)a + 1) != 0 && n_free == f0);                                               // (an interior pointer is foreign too)
        CHECK(m.release(b) != 0 && n_free == f0);                                                          // (so is a block already released)
        CHECK(m.release_all() == 0 && live.empty());
    }
    section("release");
    {
        DeviceMem m(b_alloc, b_free);
        DevBuf<int> buf;
        void* other = nullptr;
        CHECK(!m.alloc(&other, 5));
        CHECK(ensure(m, buf, 100) == 0 && buf.p && buf.cap == 100 && m.bytes() == 105);
        int a0 = n_alloc, f0 = n_free;
        int* was = buf.p;
        CHECK(ensure(m, buf, 100) == 0 && ensure(m, buf, 1) == 0 && ensure(m, buf, 0) == 0);               // cap >= bytes: no backend call
        CHECK(n_alloc == a0 && n_free == f0 && buf.p == was && buf.cap == 100);
        freed.clear();
        CHECK(ensure(m, buf, 101) == 0);                                                                  // growth: the old block goes exactly once
        CHECK(n_alloc == a0 + 1 && n_free == f0 + 1 && freed.size() == 1 && freed[0] == (void*)was && buf.cap == 101 && buf.p && m.bytes() == 106);
        CHECK(m.find(buf.p) && m.find(buf.p)->bytes == 101 && !m.find(buf.p)->user);
        fail_next = 1; f0 = n_free;
        CHECK(ensure(m, buf, 5000) != 0);                                                                 // the backend fails on growth
        CHECK(buf.p == nullptr && buf.cap == 0 && m.bytes() == 5 && n_free == f0 + 1 && m.blocks().size() == 1);
        CHECK(ensure(m, buf, 8) == 0 && buf.cap == 8 && m.bytes() == 13);                                 // ... and the next call starts over
        CHECK(m.release_all() == 0 && live.empty());
    }
    section("ensure");
    {
        DeviceMem m(b_alloc, b_free);
        void* early[2] = {};
        CHECK(!m.alloc(&early[0], 11) && !m.alloc(&early[1], 22));
        const size_t mk = m.mark(), at_mark = m.bytes();
        void* p[5] = {};
        for (int i = 0; i < 5; ++i) CHECK(!m.alloc(&p[i], 100 + i));
        CHECK(m.release(p[1]) == 0);
        freed.clear();
        CHECK(m.release_since(mk) == 0);
        std::set<void*> got(freed.begin(), freed.end());
        CHECK(freed.size() == 4 && got == (std::set<void*>{p[0], p[2], p[3], p[4]}));                     // the other four, each once
        CHECK(m.bytes() == at_mark && m.blocks().size() == 2 && m.find(early[0]) && m.find(early[1]) && live.size() == 2);
        // an earlier block released after the mark was taken: marks are not positions in the list
        const size_t mk2 = m.mark();
        void *x = nullptr, *again = nullptr;
        CHECK(!m.alloc(&x, 7));
        CHECK(m.release(early[0]) == 0);
        CHECK(!m.alloc(&again, 11));
        freed.clear();
        CHECK(m.release_since(mk2) == 0);
        got = std::set<void*>(freed.begin(), freed.end());
        CHECK(freed.size() == 2 && got == (std::set<void*>{x, again}));
        CHECK(m.bytes() == 22 && m.blocks().size() == 1 && m.find(early[1]) && live.size() == 1);
        CHECK(m.release_since(mk) == 0 && m.blocks().size() == 1);
        CHECK(m.release_since(m.mark()) == 0 && m.blocks().size() == 1);
        CHECK(m.release_all() == 0 && live.empty());
    }
    section("mark_and_release_since");
    {
        DeviceMem m(b_alloc, b_free);
        void *in0 = nullptr, *u0 = nullptr, *in1 = nullptr, *u1 = nullptr;
        CHECK(!m.alloc(&in0, 8) && !m.alloc(&u0, 16, true) && !m.alloc(&in1, 32, false) && !m.alloc(&u1, 64, true));
        CHECK(!m.find(in0)->user && m.find(u0)->user && !m.find(in1)->user && m.find(u1)->user);
        CHECK(m.find(u0)->bytes == 16 && m.find(u1)->bytes == 64);
        const int f0 = n_free;
        CHECK(m.release_all() == 0);
        CHECK(n_free == f0 + 4 && m.bytes() == 0 && m.blocks().empty() && live.empty());
        CHECK(m.release_all() == 0 && n_free == f0 + 4 && m.bytes() == 0);                                // twice: every block once
        CHECK(!m.find(u0));
        void* later = nullptr;
        CHECK(!m.alloc(&later, 3) && m.bytes() == 3);   // (the registry serves on)
        CHECK(m.release_all() == 0 && live.empty());
    }
    section("release_all_and_user_flag");
    {
        DeviceMem m(b_alloc, b_free);
        void *kept = nullptr, *lost = nullptr, *won = nullptr;
        CHECK(!m.alloc(&kept, 9));
        { AllocScope s(m); CHECK(!m.alloc(&lost, 10) && m.bytes() == 19); }                               // no commit: freed
        CHECK(m.bytes() == 9 && !m.find(lost) && m.find(kept));
        { AllocScope s(m); CHECK(!m.alloc(&won, 10)); s.commit(); }
        CHECK(m.bytes() == 19 && m.find(won));
        { ScopedBlock<double> t(m); CHECK(t.alloc(4) == 0 && t.p && m.bytes() == 19 + 32); t.p[3] = 1.0; }
        CHECK(m.bytes() == 19);
        fail_next = 1;
        { ScopedBlock<double> t(m); CHECK(t.alloc(4) != 0 && t.p == nullptr); }                           // (nothing to release)
        CHECK(m.bytes() == 19 && m.release_all() == 0 && live.empty());
    }
    section("scope_guards");
    printf("backend calls: %d alloc, %d free\n", n_alloc, n_free);
    return 0;
}
"""


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("devmem")
    (d / "probe.cpp").write_text(_PROBE)
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbb_textline_detection_amd", "csrc")
    # host pass only, the sanitizers on the host code alone, and without the HIP wrapper headers (-nogpuinc): the header must not need them
    res = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-nogpuinc", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                          "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                          "-I", csrc, str(d / "probe.cpp"), "-o", str(d / "probe")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    out = subprocess.run([str(d / "probe")], capture_output=True, text=True)      # (the leak checker is on by default)
    assert out.returncode == 0 and not out.stderr, (out.stdout[-2000:], out.stderr[-3000:])      # (a sanitizer report ends the program with a status)
    return out.stdout.splitlines()


def test_header_includes_no_hip_header():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sbb_textline_detection_amd", "csrc")
    text = open(os.path.join(csrc, "devmem.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<stddef.h>", "<vector>"], includes
    for word in ("hipMalloc(", "hipFree(", "hipError_t", "HIPCHK", "sbbseg_ctx"):
        assert word not in text, word


def test_no_check_failed(report):
    assert [line for line in report if line.startswith("FAIL")] == []


@pytest.mark.parametrize("name", SECTIONS)
def test_section(report, name):
    assert f"PASS {name}" in report, [line for line in report if line.startswith("FAIL")]
