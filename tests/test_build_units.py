"""The build finds its translation units and header dependencies by itself (funcodec_amd/build.py): what it finds is what csrc/ holds.
No GPU, no compiler."""
import glob
import os
import re

from funcodec_amd import build


def _names(pattern):
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(build.CSRC, pattern)))


def test_every_unit_is_built_exactly_once():
    units = _names("*.hip")
    assert units, "no translation units under csrc/"
    assert sorted(build.sources()) == units


def test_every_start_first_prefix_names_a_unit():
    units = _names("*.hip")
    for prefix in build.START_FIRST:
        assert any(u.startswith(prefix) for u in units), f"no unit starts with {prefix!r}"
    # the rule only orders: the units it names come first, in the rule's order
    srcs = build.sources()
    ranks = [next((i for i, p in enumerate(build.START_FIRST) if u.startswith(p)), len(build.START_FIRST)) for u in srcs]
    assert ranks == sorted(ranks)


def test_every_included_header_is_a_dependency():
    deps = {os.path.normpath(os.path.join(build.CSRC, h)) for h in build.HEADERS}
    assert all(os.path.exists(d) for d in deps)
    include = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)
    seen = 0
    for name in _names("*.hip") + _names("*.h"):
        with open(os.path.join(build.CSRC, name)) as f:
            for inc in include.findall(f.read()):
                seen += 1
                assert os.path.normpath(os.path.join(build.CSRC, inc)) in deps, f"{name} includes {inc}, which no unit depends on"
    assert seen > 0
