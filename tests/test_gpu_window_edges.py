"""GPU tests of the one anchor-scan body of dq_anchor_many.h at the edges of its windows, on all four of its routes:
new files of 1 .. 515 bytes (tests/window_edge_inputs.py: no match anywhere, so that every window runs to its last lane
and the loop ends on a head with nothing behind it; a slice of old, so that the head breaks at once; a match in the last
40 bytes, so that a lane of a window's last wave breaks) through anchor_many_kernel, anchor_mid_many_kernel and
anchor_index_many_kernel at 256 and at 512 threads.  Every patch is byte for byte the one-pair or one-file path's, its
three streams are the reference loop's, and the info call says that every file shared a launch.  (The Search count of a
file does not leave the library; tests/test_*_many*_cpu.py assert it on the same files through the window models.)"""
import numpy as np
import pytest

import window_edge_inputs as wei
from test_gpu_diff_many import streams_of

pytestmark = pytest.mark.gpu

# route -> (bytes of old, the flags that take the files through that kernel)
ROUTES = {"short": (wei.SHORT_OLD, {}),
          "medium": (wei.MEDIUM_OLD, {"DQ_DIFF_MID_MANY_MIN": "1"}),
          "index256": (wei.MEDIUM_OLD, {"DQ_INDEX_MANY_MIN": "1", "DQ_INDEX_MANY_THREADS": "256"}),
          "index512": (wei.MEDIUM_OLD, {"DQ_INDEX_MANY_MIN": "1", "DQ_INDEX_MANY_THREADS": "512"})}

_reference = {}


def reference(oracle_mod, n):
    """(old, new files, oracle.bsdiff_scan's streams of each) for the old file of n bytes, made once."""
    if n not in _reference:
        old = wei.old_file(n)
        sa = oracle_mod.divsufsort(old)
        news = [new for _, new in wei.new_files(old)]
        _reference[n] = (old, news, [oracle_mod.bsdiff_scan(old, sa, new)[:3] for new in news])
    return _reference[n]


@pytest.mark.parametrize("route", list(ROUTES))
def test_window_edges(backend_lib, oracle_mod, monkeypatch, route):
    import deltaq_amd
    from deltaq_amd import _abi
    assert backend_lib.dq_device_count() >= 1, "no MI355X visible: the HIP path cannot be tested"
    n, env = ROUTES[route]
    old, news, want_streams = reference(oracle_mod, n)
    assert sorted({x.size for x in news}) == list(wei.LENGTHS)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    if route.startswith("index"):
        with deltaq_amd.DiffIndex(old, 0) as index:
            patches = index.CreateMany(news)
            info = _abi.last_index_many_info()
            for name in env:
                monkeypatch.delenv(name)
            alone = [index.Create(new) for new in news]
        assert info["shared_files"] == len(news) and info["single_files"] == 0 and info["anchor_launches"] == 1
    else:
        patches = deltaq_amd.Diff.CreateMany([old] * len(news), news)
        info = _abi.last_diff_many_info()
        for name in env:
            monkeypatch.delenv(name)
        alone = [deltaq_amd.Diff.CreateBytes(old, new) for new in news]
        assert info["shared_pairs"] == len(news) and info["single_pairs"] == 0
        medium = route == "medium"
        assert info["medium_pairs"] == (len(news) if medium else 0)
        assert info["medium_anchor_launches"] == int(medium) and info["anchor_launches"] == int(not medium)
    for j, new in enumerate(news):
        assert patches[j] == alone[j], (route, j, new.size)
        triples, dif, extra, m = streams_of(patches[j])
        ctrl, want_dif, want_extra = want_streams[j]
        assert m == new.size, (route, j)
        assert np.array_equal(triples, ctrl), (route, j, new.size)
        assert dif == want_dif.tobytes() and extra == want_extra.tobytes(), (route, j, new.size)
