"""The polynomial routines' temporaries come out of the workspace's pool (mzk_ws.h: WsBlock) and go back into it: after a second
round of fast_zerofier / fast_evaluate / fast_interpolate over the same domain a third allocates nothing, both compute what the first
round computed, and a trim gives everything back.  Domains of 64, 65 and 1000 points: tree levels 0, 1 and 4, the smallest at which the
level scratch, the shared scratch and the retained transforms are all in use."""
import numpy as np
import pytest
import orc
from orc import FR, M128

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd
    myzkp_amd.init(0)
    return myzkp_amd


@pytest.mark.parametrize("fid", [FR, M128])
@pytest.mark.parametrize("n", [64, 65, 1000])
def test_rounds_reuse_the_pool_and_a_trim_returns_it(mz, fid, n):
    lg = 11
    root, order = orc.root_of(fid, lg), 1 << lg
    dom = orc.synth_vector(fid, 8100 + n, n)
    assert len(set(orc.from_limbs(dom))) == n
    vals = orc.synth_vector(fid, 8101 + n, n)
    poly = orc.synth_vector(fid, 8102 + n, n + 5)

    def one_round():
        out = (mz.fast_zerofier(fid, dom, root, order), mz.fast_evaluate(fid, poly, dom, root, order), mz.fast_interpolate(fid, dom, vals, root, order))
        return out, mz.workspace_bytes()

    mz.trim_workspace()
    assert mz.workspace_bytes() == 0
    first, held = one_round()
    later = [one_round() for _ in range(2)]
    print("workspace bytes after each round:", held, [h for _, h in later])
    # the first fast_interpolate leaves a cached plan behind that keeps blocks the first round's zerofier and evaluate had used, so the
    # second round may allocate those again; from then on every size class a round asks for is parked
    assert 0 < held <= later[0][1] == later[1][1]
    for got, _ in later:
        assert all(np.array_equal(a, b) for a, b in zip(got, first))
    for ref, got in zip((orc.fast_zerofier_ref(fid, dom, root, order), orc.fast_evaluate_ref(fid, poly, dom, root, order),
                         orc.fast_interpolate_ref(fid, dom, vals, root, order)), first):
        assert ref[0] == 0 and np.array_equal(got, ref[1])
    assert mz.trim_workspace() >= held
    assert mz.workspace_bytes() == 0
