"""Scratch slots are leased (myzkp_amd/csrc/mzk_ws.h): what that must not change, and the one refusal reachable through the ABI.

  growth    a slot that a larger call in between has freed and regrown serves the small call again: ntt 2^8, coset_lde to 2^12, ntt
            2^8 and fri_prove at 2^8, 2^10, 2^8 over Fr in one process -- first and third results bit for bit equal, all of them the
            oracle's / the FRI model's
  callback  mzk_fri_commit holds every round's codewords in WS_NTT_IO_A across its challenge callback; a nested mzk_ntt stages its
            input into that slot.  The nested call is refused (MZK_E_ARG, "workspace ..."), nothing of it is enqueued, and the commit
            goes on to the roots and codewords of a run whose callback does not call back in"""
import numpy as np
import pytest
import orc
import fri_prove_model as fm
from orc import FR, M128

pytestmark = pytest.mark.gpu
MZK_E_ARG = -1


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as m
    m.init(0)
    return m


def test_growth_between_calls(mz):
    w8, w12 = orc.root_of(FR, 8), orc.root_of(FR, 12)
    v = orc.synth_vector(FR, 71, 1 << 8)
    coef = orc.synth_vector(FR, 72, 1 << 10)
    first = mz.ntt(FR, w8, v)
    lde = mz.coset_lde(FR, coef, 5, w12, 1 << 12)
    third = mz.ntt(FR, w8, v)
    assert np.array_equal(first, third)
    rc, want = orc.ntt_ref(FR, w8, v)
    assert rc == 0 and np.array_equal(first, want)
    rc, want = orc.coset_ref(FR, coef, 5, w12, 1 << 12)
    assert rc == 0 and np.array_equal(lde, want)

    expansion, tests = 4, 8
    proofs = []
    for lg, seed in ((8, 73), (10, 74), (8, 73)):
        n = 1 << lg
        assert fm.num_rounds(n, expansion, tests) >= 2
        cw = orc.synth_vector(FR, seed, n)
        proof = dict(mz.fri_prove(FR, cw, orc.root_of(FR, lg), 7, expansion, tests))
        proof["last_codeword"] = orc.from_limbs(proof["last_codeword"])
        model, _ = fm.prove(fm.P_FR, orc.from_limbs(cw), orc.root_of(FR, lg), 7, expansion, tests)
        assert proof == model, lg
        proofs.append(proof)
    assert proofs[0] == proofs[2]


def test_nested_call_from_the_challenge_callback_is_refused(mz):
    n, rounds, p = 1 << 8, 3, orc.MOD[M128]
    cw = orc.synth_vector(M128, 75, n)
    omega = orc.root_of(M128, 8)
    small = orc.synth_vector(M128, 76, 1 << 6)
    refused = []

    def alpha(rnd, root):
        return int.from_bytes(orc.sha3_256(root + bytes([rnd])), "little") % p

    def plain(rnd, last, root):
        return None if last else alpha(rnd, root)

    def calls_back_in(rnd, last, root):
        if rnd == 1:
            with pytest.raises(mz.MzkError) as e:
                mz.ntt(M128, orc.root_of(M128, 6), small)
            refused.append((e.value.code, e.value.message))
        return None if last else alpha(rnd, root)

    want_cws, want_roots = mz.fri_commit(M128, cw, omega, orc.M128_GEN, rounds, plain)
    cws, roots = mz.fri_commit(M128, cw, omega, orc.M128_GEN, rounds, calls_back_in)
    assert len(refused) == 1
    code, message = refused[0]
    assert code == MZK_E_ARG and "workspace" in message, message
    assert roots == want_roots and len(roots) == rounds
    assert len(cws) == rounds and all(np.array_equal(a, b) for a, b in zip(cws, want_cws))
    assert np.array_equal(cws[0], cw)
    # outside the commit the same call is served
    rc, want = orc.ntt_ref(M128, orc.root_of(M128, 6), small)
    assert rc == 0 and np.array_equal(mz.ntt(M128, orc.root_of(M128, 6), small), want)
