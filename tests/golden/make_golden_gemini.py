"""Writes tests/golden/gemini_vectors.json: the reference's test_gemini case (gemini.rs:288-328: coef 1..8, rhos 2, 3, 4, opened at
beta = 1234) and test_sumcheck_pipeline's polynomial (sumcheck.rs:230-248) proven with the model transcript of tests/gemini_model.py,
both against setup_kzg's G1 powers (kzg.rs:27-40, max_d = 8 as the reference's tests use) for a fixed alpha.  Every point comes from
the CPU oracle (oracle/mzk_oracle.c: literal MSM, batch_open_kzg, prove_degree_bound).

    python tests/golden/make_golden_gemini.py"""
import json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np
import orc
import gemini_model as gm

ALPHA = 0x1234567890ABCDEF1122334455667788
MAX_D = 8


def arr(v):
    return orc.to_limbs(list(v), 4)


def prove_levels(fs, beta, srs):
    """commit_gemini + open_gemini of the fold levels with the oracle"""
    el = len(fs) - 1
    us = [beta, gm.neg(beta), beta * beta % gm.P]
    commits = [orc.msm_ref(arr(f), srs[:len(f)]) for f in fs]
    ys, ws = [], []
    for f in fs[:el]:
        y, w = orc.kzg_batch_open_ref(arr(f), us, srs)
        ys.append(y)
        ws.append(w)
    deg = []
    for i, f in enumerate(fs):
        rc, d = orc.kzg_degree_bound_ref(arr(f), srs, 1 << (el - i))
        assert rc == 0
        deg.append(d)
    return commits, ys, ws, deg


def main():
    srs = orc.kzg_setup_ref(ALPHA, MAX_D)
    out = {"alpha": ALPHA, "max_d": MAX_D}
    # test_gemini
    coef = list(range(1, 9))
    rhos = [2, 3, 4]
    fs = gm.split_and_fold(coef, rhos)
    c = gm.tensor_product(gm.tensor_product([1, rhos[0]], [1, rhos[1]]), [1, rhos[2]])
    mu = sum(a * b for a, b in zip(coef, c)) % gm.P
    assert fs[-1] == [mu]
    beta = 1234
    commits, ys, ws, deg = prove_levels(fs, beta, srs)
    assert gm.gemini_relation(rhos, beta, [y[0] for y in ys], [y[1] for y in ys], [y[2] for y in ys[1:]] + [mu])
    out["gemini"] = {"coef": coef, "rhos": rhos, "beta": beta, "mu": mu, "levels": fs, "commits": commits, "ys": ys, "ws": ws, "deg": deg}
    # test_sumcheck_pipeline with the model transcript
    coefs = gm.get_coefs_in_order(gm.PIPELINE_G)
    h, gs, rs, beta = gm.sumcheck_rounds(coefs)
    assert h == 41 and beta == rs[-1]
    fs = gm.split_and_fold(coefs, rs)
    commits, ys, ws, deg = prove_levels(fs, beta, srs)
    assert gm.verify_sumcheck_values(h, gs, rs, beta, ys)
    out["sumcheck"] = {"coefs": coefs, "h": h, "gs": gs, "rs": rs, "beta": beta, "levels": fs, "commits": commits, "ys": ys, "ws": ws, "deg": deg}
    path = os.path.join(HERE, "gemini_vectors.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print("wrote", path)


if __name__ == "__main__":
    main()
