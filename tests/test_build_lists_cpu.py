"""The build lists of _build.py against what csrc/ holds: a source that is not in SOURCES is never compiled (missing symbols at best),
and a header that is not in HEADERS does not make the objects that include it stale -- an edit to it leaves old objects in the library
without any error."""
import os
import re

from sbb_textline_detection_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sbb_textline_detection_amd", "csrc")


def test_every_source_and_included_header_is_in_the_build_lists():
    files = sorted(os.listdir(CSRC))
    sources = [f for f in files if f.endswith((".hip", ".cpp"))]
    assert sources and sorted(_build.SOURCES) == sources, sorted(set(sources) ^ set(_build.SOURCES))
    assert len(set(_build.SOURCES)) == len(_build.SOURCES)
    headers = {os.path.realpath(h) for h in _build.HEADERS}
    assert all(os.path.exists(h) for h in headers), [h for h in headers if not os.path.exists(h)]
    seen = 0
    for f in files:
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, f)).read(), re.M):
            # (the compile line has no -I: a quoted include is relative to the including file)
            assert os.path.realpath(os.path.join(CSRC, inc)) in headers, f"{f} includes {inc}, which _build.HEADERS does not list"
            seen += 1
    assert seen >= len(sources)                     # every unit includes at least internal.h or a header over it
