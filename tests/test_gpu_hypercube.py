"""mzk_mpoly_hypercube_evals / _dev and mzk_sumcheck_product_prove_terms / _dev through the C ABI, bit for bit against
tests/hypercube_model.py over the case table of tests/hypercube_cases.py.

  evals     every case (el = 0, 1, 2, 9, 10, 11, 12, 13: a partial tile, one tile, 2, 4 and 8 tiles; every term shape; k = 1, 2, 3, 8 and
            more; an empty factor between full ones; sums of 2^el + 64 values of p - 1) in the three forms and in the host and _dev
            entry; the _dev form between guard words on a side stream
  auto      2^13 masks in one factor: AUTO resolves to the scatter form (every other case resolves to the tile form), in evals and in prove
  dense     T = 2^el equals mzk_mle_evals_from_coeffs bit for bit
  plan      mzk_mpoly_hypercube_plan equals the model's plan on the cases
  refusals  every refusal with its code, the output untouched; n_factors == 0 writes nothing
  prove     el = 1, 7, 8, 11 (the tail alone, the first grid round, past one tile), k = 1 and 3, with and without a header, both
            entries: the packed proof equals the model's and mzk_sumcheck_product_prove's on the model's tables byte for byte; the
            refusals are those of mzk_sumcheck_product_prove"""
import ctypes, functools, random
import numpy as np
import pytest
import hypercube_cases as hc
import hypercube_model as hm
import sumcheck_product_model as sm

pytestmark = pytest.mark.gpu
P = hm.P
VP, SZ = ctypes.c_void_p, ctypes.c_size_t
FORMS = {"auto": 0, "tile": 1, "scatter": 2}
GUARD = 0xA5A5A5A55A5A5A5A
E_ARG, E_LENGTH, E_RANGE = -1, -5, -6


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as m
    m.init(0)
    return m


def limbs(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4).copy()


def arrays(factors, el):
    """term lists -> the (coefs, exps) pairs hypercube_term_table takes; duplicate rows stay"""
    out = []
    for terms in factors:
        e = np.zeros((len(terms), el), dtype=np.uint32)
        for t, (_, exps) in enumerate(terms):
            e[t, :len(exps)] = exps
        out.append((limbs([c for c, _ in terms]) if terms else np.zeros((0, 4), dtype=np.uint64), e))
    return out


@functools.lru_cache(maxsize=None)
def staged(el, name):
    """(term table, expected tables as limbs): built once, shared, never modified"""
    import myzkp_amd as m
    factors = hc.get(el, name)
    tc, te, toff, nv = m.hypercube_term_table(arrays(factors, el), el)
    want = limbs([v for table in hc.expected(el, name) for v in table]).reshape(len(factors), 1 << el, 4)
    return (tc, te, toff), len(factors), want


def p(a):
    return a.ctypes.data_as(VP)


def run_host(mz, table, k, el, form):
    tc, te, toff = table
    out = np.full((k, 1 << el, 4), GUARD, dtype=np.uint64)
    rc = mz.lib().mzk_mpoly_hypercube_evals(p(tc), p(te), toff, SZ(k), SZ(el), form, p(out))
    assert rc == 0, mz.lib().mzk_last_error()
    return out


def run_dev(mz, table, k, el, form):
    """between guard words, on a side stream"""
    import torch
    tc, te, toff = table
    words = k * (4 << el)
    buf = torch.full((4 + words + 4,), GUARD - (1 << 64), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rc = mz.lib().mzk_mpoly_hypercube_evals_dev(p(tc), p(te), toff, SZ(k), SZ(el), form, VP(buf.data_ptr() + 32), VP(side.cuda_stream))
    assert rc == 0, mz.lib().mzk_last_error()
    side.synchronize()
    got = buf.cpu().numpy().view(np.uint64)
    assert (got[:4] == GUARD).all() and (got[-4:] == GUARD).all()
    return got[4:-4].reshape(k, 1 << el, 4)


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("el,name", hc.all_cases())
def test_evals_against_the_model(mz, el, name, form, entry):
    table, k, want = staged(el, name)
    got = (run_host if entry == "host" else run_dev)(mz, table, k, el, FORMS[form])
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, "first mismatch (factor, index): %s of %d" % (bad[0], len(bad))


@functools.lru_cache(maxsize=None)
def above_the_mask_limit():
    """el = 13: every one of the 2^13 masks in one factor (above the tile form's limit of 4096 per factor), a small factor beside it"""
    el = 13
    rng = random.Random(1313)
    order = list(range(1 << el))
    rng.shuffle(order)
    factors = [[(rng.randrange(P), hc.exps_of_mask(m, el, rng)) for m in order], hc.sparse(rng, el, 19)]
    return el, factors, [hm.evals(t, el) for t in factors]


@pytest.mark.parametrize("entry", ["host", "dev"])
def test_auto_takes_the_scatter_form_above_the_mask_limit(mz, entry):
    el, factors, tables = above_the_mask_limit()
    assert mz.mpoly_hypercube_plan(arrays(factors, el), el, FORMS["auto"])["form"] == FORMS["scatter"]
    assert mz.mpoly_hypercube_plan(arrays(factors[1:], el), el, FORMS["auto"])["form"] == FORMS["tile"]
    tc, te, toff, _ = mz.hypercube_term_table(arrays(factors, el), el)
    got = (run_host if entry == "host" else run_dev)(mz, (tc, te, toff), 2, el, FORMS["auto"])
    assert np.array_equal(got, limbs([v for t in tables for v in t]).reshape(2, 1 << el, 4))


def test_prove_terms_through_the_scatter_form(mz):
    el, factors, tables = above_the_mask_limit()
    want = sm.prove(tables, 2)
    for device in (False, True):
        got = mz.sumcheck_product_prove_terms(arrays(factors, el), 2, num_vars=el, device=device)
        for key in ("sum", "evals", "challenges", "finals", "transcript"):
            assert got[key] == want[key], (key, device)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("el", [e for e in hc.ELS if e <= 11])
def test_dense_equals_mle_evals_from_coeffs(mz, el, form):
    terms = hc.get(el, "dense")[0]
    assert len(terms) == 1 << el
    coef = [0] * (1 << el)
    for c, exps in terms:
        coef[hm.mask_of(exps, el)] = c
    butterfly = mz.mle_evals_from_coeffs(limbs(coef))
    table, k, _ = staged(el, "dense")
    assert np.array_equal(run_host(mz, table, k, el, FORMS[form])[0], butterfly)


@pytest.mark.parametrize("el", hc.ELS)
def test_plan_through_the_abi(mz, el):
    for name in ("shapes", "k8_unequal_counts", "empty_between_full"):
        factors = hc.get(el, name)
        for form in (0, 1, 2):
            got = mz.mpoly_hypercube_plan(arrays(factors, el), el, form)
            want = hm.plan([[e for _, e in f] for f in factors], el, form)
            for key in ("form", "terms", "max_masks", "max_groups", "launches", "memsets", "grid_x", "grid_y", "mle_passes", "upload_bytes", "workspace_bytes",
                        "table_bytes"):
                assert got[key] == want[key], (name, form, key)
            assert got["tile_log"] == want["g"]
            assert got["factor_masks"] == [len(f["masks"]) for f in want["factors"]][:8]
            assert got["factor_groups"] == [len(f["groups"]) for f in want["factors"]][:8]
            assert got["masks"] == sum(len(f["masks"]) for f in want["factors"])


def test_refusals_leave_the_output_untouched(mz):
    import torch
    L = mz.lib()
    el, k = 4, 2
    factors = [[(3, (1, 0, 0, 2)), (P - 1, (0, 0, 0, 0))], [(5, (0, 1, 1, 0))]]
    tc, te, toff, _ = mz.hypercube_term_table(arrays(factors, el), el)
    out = np.full((k, 1 << el, 4), GUARD, dtype=np.uint64)
    dev = torch.full((k * (4 << el) + 2,), GUARD - (1 << 64), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    bad_coef = tc.copy()
    bad_coef[2] = limbs([P])[0]
    down = (ctypes.c_size_t * 3)(2, 3, 1)
    huge = (ctypes.c_size_t * 2)(0, 1 << 28)

    def host(c=tc, e=te, o=toff, nf=k, nv=el, form=0, t=out):
        return L.mzk_mpoly_hypercube_evals(None if c is None else p(c), None if e is None else p(e), o, SZ(nf), SZ(nv), form, None if t is None else p(t))

    def devf(c=tc, e=te, o=toff, nf=k, nv=el, form=0, t=dev.data_ptr()):
        return L.mzk_mpoly_hypercube_evals_dev(None if c is None else p(c), None if e is None else p(e), o, SZ(nf), SZ(nv), form, VP(t), VP(stream))
    for f in (host, devf):
        assert f(c=None) == E_ARG and f(e=None) == E_ARG and f(o=None) == E_ARG and f(t=None) == E_ARG
        assert f(form=3) == E_ARG and f(form=-1) == E_ARG
        assert f(nv=31) == E_LENGTH
        assert f(o=down) == E_LENGTH
        assert f(o=huge, nf=1) == E_LENGTH
        assert f(c=bad_coef) == E_RANGE
        assert f(nf=0) == 0
    assert devf(t=dev.data_ptr() + 8) == E_ARG
    from myzkp_amd._lib import _HypercubePlan
    plan = _HypercubePlan()
    assert L.mzk_mpoly_hypercube_plan(p(te), toff, SZ(k), SZ(el), 0, None) == E_ARG
    assert L.mzk_mpoly_hypercube_plan(p(te), down, SZ(k), SZ(el), 0, ctypes.byref(plan)) == E_LENGTH
    assert L.mzk_mpoly_hypercube_plan(p(te), toff, SZ(k), SZ(el), 7, ctypes.byref(plan)) == E_ARG
    torch.cuda.synchronize()
    assert (out == GUARD).all() and (dev.cpu().numpy().view(np.uint64) == GUARD).all()
    # and the same arguments without a fault are accepted
    assert host() == 0 and devf() == 0
    torch.cuda.synchronize()
    want = limbs([v for f in factors for v in hm.evals(f, el)]).reshape(k, 1 << el, 4)
    assert np.array_equal(out, want) and np.array_equal(dev.cpu().numpy().view(np.uint64)[:-2].reshape(k, 1 << el, 4), want)


# ---- the prover from term tables -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def prove_case(el, k, with_header):
    """(factors, model tables, d, header objects, the model's proof): computed once, shared, never modified.  Exponents up to 4: every
    factor is non-multilinear"""
    rng = random.Random(500 + 10 * el + k)
    factors = [hc.sparse(rng, el, 5 + 9 * f) + [(rng.randrange(P), ())] for f in range(k)]
    tables = [hm.evals(t, el) for t in factors]
    d = max(k, 2)
    header = ()
    if with_header:
        header = tuple(tuple(o) for o in sm.reference_header(d, k, el, [bytes(rng.randrange(256) for _ in range(9 + 4 * f)) for f in range(k)]))
    return factors, tables, d, header, sm.prove(tables, d, header)


def written(mz, el, k, d, header_len, raw):
    sec, _ = mz.sumcheck_product_layout(el, k, d, header_len)
    at = sec["transcript_len"][0]
    return raw[:sec["transcript"][0] + int.from_bytes(raw[at:at + 8], "little")]


@pytest.mark.parametrize("with_header", [False, True])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("el", [1, 7, 8, 11])
def test_prove_terms(mz, el, k, with_header):
    factors, tables, d, header, want = prove_case(el, k, with_header)
    hlen = len(mz.sumcheck_frame_header(header))
    from_tables = mz.sumcheck_product_prove(np.stack([limbs(t) for t in tables]), d, header_objects=header, raw=True)
    for device in (False, True):
        raw = mz.sumcheck_product_prove_terms(arrays(factors, el), d, header_objects=header, num_vars=el, device=device, raw=True)
        got = mz.sumcheck_product_unpack(el, k, d, hlen, raw)
        for key in ("sum", "evals", "challenges", "finals", "transcript"):
            assert got[key] == want[key], (key, device)
        assert written(mz, el, k, d, hlen, raw) == written(mz, el, k, d, hlen, from_tables)


def test_prove_terms_refusals_are_those_of_the_prover(mz):
    L = mz.lib()
    el, k, d = 3, 2, 2
    factors, tables, _, _, _ = prove_case(3, 2, False)
    tc, te, toff, _ = mz.hypercube_term_table(arrays(factors, el), el)
    tab = np.stack([limbs(t) for t in tables])
    hdr = mz.sumcheck_frame_header([[b"abc"]])
    hbuf = (ctypes.c_uint8 * len(hdr)).from_buffer_copy(hdr)
    _, total = mz.sumcheck_product_layout(el, k, d, len(hdr))
    proof = np.full(total + 64, 0x5A, dtype=np.uint8)

    def both(nf=k, nv=el, deg=d, h=hbuf, hl=len(hdr), ho=1, out=proof, cap=total + 64):
        o = None if out is None else p(out)
        tail = (SZ(deg), h, SZ(hl), SZ(ho), o, SZ(cap))
        offs = toff if nf <= k else (ctypes.c_size_t * (nf + 1))(*([0] * (nf + 1)))
        a = L.mzk_sumcheck_product_prove_terms(p(tc), p(te), offs, SZ(nf), SZ(nv), *tail)
        b = L.mzk_sumcheck_product_prove(p(tab), SZ(nv), SZ(nf), *tail)
        return a, b
    for kw, code in [(dict(nv=0), E_LENGTH), (dict(nv=31), E_LENGTH), (dict(nf=0), E_ARG), (dict(nf=9), E_ARG), (dict(deg=0), E_ARG), (dict(deg=9), E_ARG),
                     (dict(ho=2), E_ARG), (dict(hl=len(hdr) - 1), E_ARG), (dict(h=None), E_ARG), (dict(out=None), E_ARG), (dict(cap=total - 1), E_LENGTH)]:
        assert both(**kw) == (code, code), kw
    assert (proof == 0x5A).all()
    bad = tc.copy()
    bad[0] = limbs([P])[0]
    assert L.mzk_sumcheck_product_prove_terms(p(bad), p(te), toff, SZ(k), SZ(el), SZ(d), hbuf, SZ(len(hdr)), SZ(1), p(proof), SZ(total)) == E_RANGE
    assert L.mzk_sumcheck_product_prove_terms(None, p(te), toff, SZ(k), SZ(el), SZ(d), hbuf, SZ(len(hdr)), SZ(1), p(proof), SZ(total)) == E_ARG
    assert (proof == 0x5A).all()
    import torch
    dproof = torch.zeros(total + 8, dtype=torch.uint8, device="cuda")
    args = (p(tc), p(te), toff, SZ(k), SZ(el), SZ(d), hbuf, SZ(len(hdr)), SZ(1))
    assert L.mzk_sumcheck_product_prove_terms_dev(*args, VP(dproof.data_ptr() + 4), SZ(total), VP(torch.cuda.current_stream().cuda_stream)) == E_ARG
    assert both() == (0, 0)
