"""The memory contract of smooth_tracks (tests/guarded.py run_contract): every guard of every output and of
the workspace intact, every element of all seven returned tensors written (no exemption), the same bits under both prefills and
both surroundings of the inputs and the bits of the plain call, the inputs handed to the launch uncopied, the workspace among the
guarded uint8 allocations.  (T,J) = (130,3) in segments (1,129): a track of one frame beside a split track whose last block holds
two frames, with gaps and NaN points, so that passed-through, one-lane and split tracks write side by side."""
import numpy as np
import pytest

from tests import guarded as G
from tests import smooth_tracks_cases as sc

pytestmark = pytest.mark.gpu

EXEMPT = {}


@pytest.mark.parametrize("mode", ["plain", "huber"])
def test_smooth_tracks_contract(mode, capsys):
    from openmpl_amd import cabi, smooth_tracks
    T, J, seg = 130, 3, (1, 129)
    c = sc.case(T, J, segments=seg, weights="mixed", gaps="middle40", nan_points=True, outliers=True)
    kw = dict(smoothness=1.0, order=2, huber=sc.HUBER if mode == "huber" else None)
    ws = cabi.load().mpl_smooth_tracks_workspace_bytes(T, J, len(seg))
    assert ws > 0
    args = dict(points=np.array(c["points"]), weight=np.array(c["weight"]))
    r, n, b = G.run_contract(lambda **a: smooth_tracks(segments=seg, **a, **kw), args, exempt=EXEMPT, workspace_bytes=(ws,), min_outputs=7)
    assert r.points64 is None and int(r.status.max()) <= 2 and int(r.iterations.max()) <= 20
    st = r.status.cpu().numpy()
    assert (st[0] == 2).all() or kw["order"] == 1          # one frame cannot take part twice: the first segment passes through
    with capsys.disabled():
        print("\nsmooth_tracks %s: %d guarded allocations, %d bytes (run three times between its guards)" % (mode, n, b))
