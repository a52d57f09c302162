"""CPU: what build() watches is what the one translation unit reads, and fql_amd/csrc stays flat.

build() recompiles when fql_engine.hip or a header of HDRS is newer than the library, so a header the unit includes and HDRS lacks
leaves a stale library behind an edit.  bench.py hashes every entry of fql_amd/csrc with open(): a subdirectory there ends every
benchmark run.  No GPU, no compile."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
CSRC = os.path.join(ROOT, 'fql_amd', 'csrc')


def reachable(src):
    """src and every file a quoted #include reaches from it, transitively; each must be a file inside the repository."""
    seen, todo = set(), [os.path.realpath(src)]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', open(f).read(), re.M):
            p = os.path.realpath(os.path.join(os.path.dirname(f), inc))
            # the unit's quoted includes are all its own files, named relative to the includer: one that is not there is a wrong path
            assert os.path.isfile(p) and p.startswith(os.path.realpath(ROOT) + os.sep), (f, inc)
            todo.append(p)
    return seen


def test_every_included_file_is_a_build_input():
    import __graft_entry__ as G
    inputs = {os.path.realpath(p) for p in [G.SRC] + G.HDRS}
    files = reachable(G.SRC)
    for name in ('fql_amd/csrc/fql_kernels.h', 'fql_amd/csrc/fql_engine_groups.h', 'include/fql_amd.h'):   # the walk does follow the includes
        assert os.path.realpath(os.path.join(ROOT, name)) in files, name
    assert not files - inputs, sorted(files - inputs)


def test_csrc_is_flat():
    for name in sorted(os.listdir(CSRC)):
        p = os.path.join(CSRC, name)
        assert os.path.isfile(p) and not os.path.islink(p), name


def test_source_hash_reads_every_entry():
    import pmc_summary
    assert re.fullmatch(r'[0-9a-f]{16}', pmc_summary.source_sha16(ROOT))
