"""mzk_stark_prove at every AIR shape of tests/stark_shape_cases.py against the model's prover (tests/stark_model.py, Python integers),
bit for bit.  tests/test_gpu_stark.py pins the one call to the model at the reference's parameters only (two registers, degree 2,
expansion 4, two equal shifts); here the register count, the constraint degree and count, the expansion factor, the number of
colinearity checks, the boundary and the field vary, so that the buffers laid out by m, every shift, the prefix interpolation and
the prefix zerofier, the host branch of the coset division, the tail fill of a short trace polynomial, the empty boundary quotient
and FRI, the trees and the openings at domains of 32 to 2048 elements are all reached (tests/test_stark_shape_cases.py shows on the
CPU which case reaches what, and that a mismatch here is not the table's fault).  Per case:
  * the handle's plan, its transition-zerofier root and its roots of unity are the model's;
  * the one call -- host form twice, _dev form once, identical bytes -- gives the model's proof section by section, and the indices;
  * the stage entry points at the same arguments give the model's intermediates and the same proof;
  * the model's verifier accepts the library's proof, rejects it with one value, path byte or root changed in any section, and
    answers "combination" to the library's proof of a false boundary.
Then a refusal AFTER work was enqueued (a transition polynomial that composes to zero: the coset division's documented
MZK_E_LENGTH) leaves the handle and the workspace usable, and one handle proves three boundaries with different root counts."""
import numpy as np
import pytest
import orc
import stark_model as sm
import stark_shape_cases as C
from test_gpu_stark_stages import env, prove_staged     # noqa: F401 (env is a fixture)
from test_gpu_stark import limbs_trace, prove_both, tampered

pytestmark = pytest.mark.gpu


def handle(mz, b):
    c = b.case
    return mz.Stark(b.fid, c.e, c.checks, c.m, c.T, c.deg, b.g, b.cons)


def assert_equals_model(proof, want, what):
    """the FastStarkProof section by section, then as a whole"""
    fri, wfri = proof["fri"], want["fri"]
    assert fri["merkle_roots"] == wfri["merkle_roots"], "%s: fri.merkle_roots" % what
    assert fri["last_codeword"] == wfri["last_codeword"], "%s: fri.last_codeword" % what
    assert fri["top_level_indices"] == wfri["top_level_indices"], "%s: fri.top_level_indices" % what
    assert len(fri["revealed_layers"]) == len(wfri["revealed_layers"]), "%s: fri.revealed_layers" % what
    for i, (got, exp) in enumerate(zip(fri["revealed_layers"], wfri["revealed_layers"])):
        for kind in "abc":
            assert list(got[kind][0]) == list(exp[kind][0]), "%s: fri layer %d %s values" % (what, i, kind)
            assert [list(q) for q in got[kind][1]] == [list(q) for q in exp[kind][1]], "%s: fri layer %d %s paths" % (what, i, kind)
    assert proof["bqc_roots"] == want["bqc_roots"], "%s: bqc_roots" % what
    assert proof["rdc_root"] == want["rdc_root"], "%s: rdc_root" % what
    for key in ("bqc_points", "rdc_points", "tzc_points"):
        assert list(proof[key]) == list(want[key]), "%s: %s" % (what, key)
    for key in ("bqc_paths", "rdc_paths", "tzc_paths"):
        assert [list(q) for q in proof[key]] == [list(q) for q in want[key]], "%s: %s" % (what, key)
    assert sm.proof_digest(proof) == sm.proof_digest(want), "%s: digest" % what


def prove_and_compare(env, st, b, want, what):
    mz = env[1]
    raw, proof = prove_both(env, st, b.fid, b.trace, b.boundary, b.randomizer)
    assert len(raw) == sm.proof_layout(C.LIMBS[b.fid], b.plan)[1], what
    assert_equals_model(proof, want, what)
    assert mz.stark_unpack_proof(b.fid, b.plan, raw)["indices"] == want["_debug"]["indices"], "%s: indices" % what
    return proof


@pytest.mark.parametrize("name", C.VERIFYING)
def test_prove_equals_the_model(env, name):
    mz = env[1]
    b = C.build(name)
    c, d = b.case, b.plan
    want = C.model_proof(name)
    dbg = want["_debug"]
    tz_root = dbg["transition_zerofier_root"]
    assert mz.root_of_unity(b.fid, d["omicron_domain_length"].bit_length() - 1) == b.omicron
    assert mz.root_of_unity(b.fid, d["fri_domain_length"].bit_length() - 1) == b.omega
    with handle(mz, b) as st:
        assert st.dims(b.boundary) == d
        assert st.transition_zerofier_root() == tz_root
        proof = prove_and_compare(env, st, b, want, name)
        # the stages at the same arguments, every intermediate against the model's.  A constant register's polynomials are shorter than their
        # degree bounds, which the staged helper otherwise asserts to be met exactly.
        staged, extra = prove_staged(env, b.fid, b.p, b.g, b.omega, b.omicron, c.e, c.checks, c.m, c.T, c.deg, b.cons, b.trace, b.boundary, b.randomizer,
                                     dbg=dbg, exact=c.kind != "constant")
        assert extra["dims"] == d and extra["tz_root"] == tz_root
        assert sm.proof_digest(staged) == sm.proof_digest(proof), "the stages and the one call differ"
        assert b.model.verify(proof, b.air, b.boundary, tz_root) is True
        for key, bad in tampered(proof, b.p):
            assert b.model.verify(bad, b.air, b.boundary, tz_root) is not True, key
        _, false_proof = prove_both(env, st, b.fid, b.trace, b.false_boundary, b.randomizer)
        assert b.model.verify(false_proof, b.air, b.false_boundary, tz_root) == "combination"


def test_refusal_after_work_is_enqueued_leaves_the_handle_usable(env):
    """R1: next1 - prev1 of a constant register composes to the zero polynomial, which the coset division refuses (ntt.rs:285) when the
    interpolation, the boundary division, the extensions and m + 1 trees of this prove are already enqueued or built"""
    torch, mz, dev, stream = env
    b, then = C.build(C.REFUSED.name), C.build(C.REFUSED_THEN.name)
    want = C.model_proof(C.REFUSED_THEN.name)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).to(dev)
    with handle(mz, b) as st:
        t, r = limbs_trace(b.fid, b.trace), orc.to_limbs(b.randomizer, C.LIMBS[b.fid])
        _, total = mz.stark_proof_layout(b.fid, st.dims(b.boundary))
        d_t, d_r = to_dev(t), to_dev(r)
        d_p = torch.zeros(total + 8, dtype=torch.uint8, device=dev)
        for call in (lambda: st.prove_raw(t, b.boundary, r),
                     lambda: st.prove_dev(d_t.data_ptr(), len(b.trace), b.boundary, d_r.data_ptr(), d_p.data_ptr(), total, stream)):
            with pytest.raises(mz.MzkError) as e:
                call()
            assert e.value.code == -5 and "rhs.degree() < lhs.degree()" in e.value.message
        torch.cuda.synchronize()
        prove_and_compare(env, st, then, want, "after the refusal")
        with pytest.raises(mz.MzkError) as e:
            st.prove_raw(t, b.boundary, r)
        assert e.value.code == -5
        assert mz.trim_workspace() >= 0
        prove_and_compare(env, st, then, want, "after the refusal and the trim")


def test_one_handle_three_boundaries(env):
    """the per-call plan and root lists carry no state: 2 + 1, 0 + 1 and 3 + 0 boundary entries per register, one after the other, and the
    first again"""
    mz = env[1]
    with handle(mz, C.build(C.REUSE_ROW)) as st:
        for cells in list(C.REUSE_BOUNDARIES) + [C.REUSE_BOUNDARIES[0]]:
            b = C.build(C.REUSE_ROW, cells)
            assert st.dims(b.boundary) == b.plan
            prove_and_compare(env, st, b, C.model_proof(C.REUSE_ROW, cells), "boundary counts %s" % b.plan["boundary_counts"])
