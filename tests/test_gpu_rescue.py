"""mzk_rescue_* (the RescuePrime class): Rescue-Prime hashes, chains and traces on the device against tests/rescue_cases.py's model.
  * the reference's parameters: its two known answers and the inputs 0, 1, p - 1, p - 2; the ten-link chain of test_fast_stark link by link;
  * every (m, n_rounds) cell over M128, m in {1, 2, 4} with n in {1, 3} over Fr; the exponent shapes and the states that pass through zero;
  * batches of 1, 63, 64, 65, 257, 4099 and one wave past the plan's grid cap, every lane with its own input;
  * chains of 1, 2 and 10 links; hash == trace's outputs == row n_rounds, element 0;
  * the trace layout: a stride of exactly the rows, a stride with 8 more rows whose pattern survives, guard elements, outputs = NULL, host
    forms against _dev forms; a side stream behind a torch kernel that writes the inputs; every refusal with nothing written; workspace;
  * preimage to proof on one stream: trace_dev into a buffer that already holds the random rows, Stark.prove_dev behind it without a
    synchronisation, the proof byte for byte the one from the model's host trace, accepted by stark_model.verify -- for one input and for
    three slots of one trace buffer proved one after another."""
import ctypes, random
import numpy as np
import pytest
import rescue_cases as rc

pytestmark = pytest.mark.gpu
MASK = (1 << 64) - 1
GUARD = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def env():
    import torch
    import myzkp_amd as mz
    mz.init(0)
    return torch, mz, torch.device("cuda", 0)


def fid_of(mz, c):
    return mz.FIELD_M128 if c["field"] == "m128" else mz.FIELD_FR


def handle(mz, c):
    return mz.RescuePrime(fid_of(mz, c), c["m"], c["n"], c["alpha"], c["alphainv"], c["mds"], c["rc"])


def ints(a):
    """(count x limbs) uint64 -> Python ints"""
    a = np.asarray(a, dtype=np.uint64)
    a = a.reshape(-1, a.shape[-1])
    cols = [a[:, j].tolist() for j in range(a.shape[1])]
    return [sum(c[i] << (64 * j) for j, c in enumerate(cols)) for i in range(a.shape[0])]


def limbs(vals, nl):
    return np.array([[(int(v) >> (64 * j)) & MASK for j in range(nl)] for v in vals], dtype=np.uint64).reshape(len(vals), nl)


def to_dev(torch, dev, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).to(dev)


def from_dev(t, nl):
    return t.cpu().numpy().view(np.uint64).reshape(-1, nl)


def check_case(env, c, inputs=None, links=None):
    """hash, trace (host forms) and both _dev forms of one case against the model"""
    torch, mz, dev = env
    nl = rc.LIMBS[c["field"]]
    inputs = c["inputs"] if inputs is None else inputs
    links = c["links"] if links is None else links
    rows, m = c["n"] + 1, c["m"]
    want = [rc.model_chain(c, x, links) for x in inputs]
    want_out = [o for ch in want for _, o in ch]
    want_tr = [v for ch in want for t, _ in ch for row in t for v in row]
    with handle(mz, c) as h:
        assert ints(h.hash(inputs, links)) == want_out, c["name"]
        tr, out = h.trace(inputs, links)
        assert tr.shape == (len(inputs) * links, rows * m, nl) and ints(tr.reshape(-1, nl)) == want_tr, c["name"]
        assert ints(out) == want_out, c["name"]
        d_in = to_dev(torch, dev, limbs(inputs, nl))
        d_out = torch.zeros(len(want_out) * nl, dtype=torch.int64, device=dev)
        d_out2 = torch.zeros_like(d_out)
        d_tr = torch.zeros(len(want_tr) * nl, dtype=torch.int64, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        h.hash_dev(d_in.data_ptr(), len(inputs), links, d_out.data_ptr(), s)
        h.trace_dev(d_in.data_ptr(), len(inputs), links, d_tr.data_ptr(), rows * m, d_out2.data_ptr(), s)
        torch.cuda.synchronize()
        assert ints(from_dev(d_out, nl)) == want_out and ints(from_dev(d_out2, nl)) == want_out and ints(from_dev(d_tr, nl)) == want_tr, c["name"]
        assert ints(from_dev(d_in, nl)) == [int(x) for x in inputs], "the inputs were written"
    return want


def test_known_answers_of_the_reference(env):
    g = rc.golden()
    c = rc.BY_NAME["reference"]
    p = rc.M128_P
    assert c["inputs"][2:] == [0, 1, p - 1, p - 2]
    want = check_case(env, c)
    for k, kat in zip(range(2), g["kats"]):
        assert c["inputs"][k] == int(kat["input"]) and want[k][0][1] == int(kat["hash"])


CELLS = ["m128-m%d-n%d" % (m, n) for m in (1, 2, 3, 4) for n in (1, 2, 27, 64)] + ["fr-m%d-n%d" % (m, n) for m in (1, 2, 4) for n in (1, 3)]


@pytest.mark.parametrize("name", CELLS)
def test_every_cell(env, name):
    check_case(env, rc.BY_NAME[name])


def test_exponent_shapes(env):
    seen = 0
    for c in rc.CASES:
        if "-exp-" in c["name"]:
            check_case(env, c, inputs=c["inputs"] + [0, 1, rc.PRIME[c["field"]] - 1])
            seen += 1
    assert seen == len(rc.ALPHAS) * len(rc.ALPHAINVS_M128) + len(rc.ALPHAINVS_FR)


@pytest.mark.parametrize("name", ["zero-all", "zero-backward", "zero-one-element"])
def test_states_that_pass_through_zero(env, name):
    c = rc.BY_NAME[name]
    want = check_case(env, c)
    if name == "zero-all":
        assert all(v == 0 for t, _ in want[0] for row in t for v in row)
    if name == "zero-backward":
        assert want[0][0][1] == c["rc"][1]


# ---- batches: every lane its own input ----------------------------------------------------------------------------------------------------
BATCH_CASE = rc.seeded("batch", "m128", 1, 1, 3, 5, 4242, n_inputs=0)       # two cheap S-boxes: half a million hashes stay a second of Python
_batch_ref = {}


def batch_reference(n):
    """inputs (n x 2 uint64, seeded, below p) and the model's outputs, computed once for the largest batch asked for so far"""
    if "n" not in _batch_ref or _batch_ref["n"] < n:
        size = max(n, 4099)                     # at most two references: the small batches share one, the batch past the cap is its own
        rng = np.random.default_rng(77)
        a = np.empty((size, 2), dtype=np.uint64)
        a[:, 0] = rng.integers(0, 1 << 63, size=size, dtype=np.uint64) * 2 + rng.integers(0, 2, size=size, dtype=np.uint64)
        a[:, 1] = rng.integers(0, 0xcb80000000000000, size=size, dtype=np.uint64)        # below the top word of p
        a[0], a[1] = (0, 0), (1, 0)
        xs = ints(a)
        p, c = rc.M128_P, BATCH_CASE
        k, r0, r1 = c["mds"][0][0], c["rc"][0], c["rc"][1]
        outs = [(k * pow((k * pow(x, 3, p) + r0) % p, 5, p) + r1) % p for x in xs]
        assert outs[:3] == [rc.model_hash(c, x) for x in xs[:3]]
        _batch_ref.update(n=size, a=a, out=limbs(outs, 2))
    return _batch_ref["a"][:n], _batch_ref["out"][:n]


def cap_batch(mz):
    c = BATCH_CASE
    pl = mz.rescue_plan(mz.FIELD_M128, c["m"], c["n"], c["alpha"], c["alphainv"], 1)
    return pl["grid_cap"] * pl["block"] + pl["block"]


@pytest.mark.parametrize("batch", [1, 63, 64, 65, 257, 4099, "one wave past the grid cap"])
def test_batch_sizes(env, batch):
    """The cap is reachable: 8192 workgroups of 64 chains of two S-boxes are milliseconds on the device; the second round of the grid
    then holds exactly one workgroup."""
    torch, mz, dev = env
    n = cap_batch(mz) if isinstance(batch, str) else batch
    pl = mz.rescue_plan(mz.FIELD_M128, 1, 1, 3, 5, n)
    assert pl["iters"] == (2 if isinstance(batch, str) else 1) and pl["grid"] * pl["iters"] >= pl["wgs"]
    a, want = batch_reference(n)
    with handle(mz, BATCH_CASE) as h:
        d_in = to_dev(torch, dev, a)
        d_out = torch.full(((n + 2) * 2,), GUARD, dtype=torch.int64, device=dev)       # one guard element on either side
        h.hash_dev(d_in.data_ptr(), n, 1, d_out.data_ptr() + 16, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = from_dev(d_out, 2)
        assert np.array_equal(got[1:n + 1], want)
        assert (got[0] == GUARD).all() and (got[n + 1] == GUARD).all()
        if n <= 4099:
            assert np.array_equal(h.hash(a), want)


# ---- chains ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("links", [1, 2, 10])
def test_chains(env, links):
    torch, mz, dev = env
    c = rc.BY_NAME["reference-chain"]
    inputs = [rc.CHAIN_INPUT, 0, 987654321987654321]
    want = [rc.model_chain(c, x, links) for x in inputs]
    rows, m = c["n"] + 1, c["m"]
    with handle(mz, c) as h:
        out = ints(h.hash(inputs, links))
        tr, tout = h.trace(inputs, links)
        tr = np.asarray(ints(tr.reshape(-1, 2)), dtype=object).reshape(len(inputs), links, rows, m)
        assert ints(tout) == out
        for b in range(len(inputs)):
            for l in range(links):
                t, o = want[b][l]
                assert out[b * links + l] == o == tr[b, l, rows - 1, 0], (b, l)            # hash == outputs == row n_rounds, element 0
                assert tr[b, l].tolist() == t, (b, l)
                if l:
                    assert tr[b, l, 0].tolist() == [want[b][l - 1][1], 0]


# ---- the trace layout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra_rows", [0, 8])
def test_trace_layout(env, extra_rows):
    torch, mz, dev = env
    c = rc.BY_NAME["m128-m3-n2"]
    nl, m, rows, links = 2, c["m"], c["n"] + 1, 2
    inputs = c["inputs"]
    slots, stride = len(inputs) * links, (rows + extra_rows) * m
    want = [rc.model_chain(c, x, links) for x in inputs]
    want_out = [o for ch in want for _, o in ch]
    pattern = np.arange(slots * stride * nl, dtype=np.uint64).reshape(slots, stride, nl) * np.uint64(0x9E3779B97F4A7C15) | np.uint64(1 << 63)
    expect = pattern.copy()
    for b, ch in enumerate(want):
        for l, (t, _) in enumerate(ch):
            expect[b * links + l, :rows * m] = limbs([v for row in t for v in row], nl)
    with handle(mz, c) as h:
        # host form: what lies behind the rows of a slot survives
        tr, out = h.trace(inputs, links, trace_stride=stride, traces=pattern.copy())
        assert np.array_equal(tr, expect) and ints(out) == want_out
        tr2, none = h.trace(inputs, links, trace_stride=stride, traces=pattern.copy(), with_outputs=False)          # outputs = NULL
        assert none is None and np.array_equal(tr2, expect)
        # _dev form, guard elements before and after the buffer
        g = 3
        buf = np.full((slots * stride + 2 * g, nl), GUARD, dtype=np.uint64)
        buf[g:-g] = pattern.reshape(-1, nl)
        d_tr = to_dev(torch, dev, buf)
        d_in = to_dev(torch, dev, limbs(inputs, nl))
        d_out = torch.zeros(slots * nl, dtype=torch.int64, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        h.trace_dev(d_in.data_ptr(), len(inputs), links, d_tr.data_ptr() + g * 8 * nl, stride, d_out.data_ptr(), s)
        torch.cuda.synchronize()
        got = from_dev(d_tr, nl)
        assert (got[:g] == GUARD).all() and (got[-g:] == GUARD).all()
        assert np.array_equal(got[g:-g].reshape(slots, stride, nl), expect)
        assert ints(from_dev(d_out, nl)) == want_out
        d_tr2 = to_dev(torch, dev, buf)
        h.trace_dev(d_in.data_ptr(), len(inputs), links, d_tr2.data_ptr() + g * 8 * nl, stride, None, s)             # d_outputs = NULL
        torch.cuda.synchronize()
        assert np.array_equal(from_dev(d_tr2, nl), got)


def test_dev_form_on_a_side_stream_behind_a_torch_kernel(env):
    torch, mz, dev = env
    c = rc.BY_NAME["reference"]
    inputs = c["inputs"]
    want = [rc.model_hash(c, x) for x in inputs]
    src = to_dev(torch, dev, limbs(inputs, 2))
    d_in = torch.zeros_like(src)
    d_out = torch.zeros_like(src)
    a = torch.randn(2048, 2048, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with handle(mz, c) as h:
        with torch.cuda.stream(side):
            b = a @ a                      # keeps the stream busy in front of the copy that writes the inputs
            d_in.copy_(src + (b[0, 0] * 0).to(torch.int64))
            h.hash_dev(d_in.data_ptr(), len(inputs), 1, d_out.data_ptr(), side.cuda_stream)
        side.synchronize()
        assert ints(from_dev(d_out, 2)) == want


def test_refusals_enqueue_nothing_and_workspace(env):
    torch, mz, dev = env
    c = rc.BY_NAME["m128-m2-n2"]
    p, nl, m, n = rc.M128_P, 2, 2, 2
    SZ, VP = ctypes.c_size_t, ctypes.c_void_p
    L = mz.lib()

    def refused(fn, code, text):
        with pytest.raises(mz.MzkError) as e:
            fn()
        assert e.value.code == code and text in e.value.message, (e.value.code, e.value.message)

    mk = lambda **kw: mz.RescuePrime(**dict(dict(fid=mz.FIELD_M128, m=m, n=n, alpha=3, alphainv=5, mds=c["mds"], round_constants=c["rc"]), **kw))
    refused(lambda: mk(fid=mz.FIELD_FQ), -1, "field id 2")
    refused(lambda: mk(fid=3), -1, "field id 3")
    refused(lambda: mk(m=0), -1, "m = 0")
    refused(lambda: mk(m=5), -1, "m = 5")
    refused(lambda: mk(n=0), -1, "n_rounds = 0")
    refused(lambda: mk(n=65), -1, "n_rounds = 65")
    refused(lambda: mk(mds=[[1, 2], [3, p]]), -6, "mds[3]")
    refused(lambda: mk(round_constants=c["rc"][:5] + [p + 1] + c["rc"][6:]), -6, "round_constants[5]")
    one = mz.to_limbs([1], 4)
    h0 = VP()
    assert L.mzk_rescue_new(1, SZ(m), SZ(n), ctypes.c_uint64(3), None, one.ctypes.data_as(VP), one.ctypes.data_as(VP), ctypes.byref(h0)) == -1
    assert L.mzk_rescue_new(1, SZ(1), SZ(1), ctypes.c_uint64(3), one.ctypes.data_as(VP), None, one.ctypes.data_as(VP), ctypes.byref(h0)) == -1
    assert L.mzk_rescue_new(1, SZ(1), SZ(1), ctypes.c_uint64(3), one.ctypes.data_as(VP), one.ctypes.data_as(VP), one.ctypes.data_as(VP), None) == -1
    inputs = c["inputs"]
    x = limbs(inputs, nl)
    mz.RescuePrime(mz.FIELD_M128, m, n, 3, 5, c["mds"], c["rc"]).hash(inputs)        # the host forms' scratch exists from here on
    w0 = mz.workspace_bytes()
    h = handle(mz, c)
    rows = n + 1
    d_in = to_dev(torch, dev, x)
    d_out = torch.full((64,), 7, dtype=torch.int64, device=dev)
    d_tr = torch.full((1024,), 7, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    big = 1 << 62
    for fn, code, text in (
            (lambda: h.hash([p]), -6, "inputs[0] not canonical"),
            (lambda: h.hash(inputs[:2] + [p + 5]), -6, "inputs[2] not canonical"),
            (lambda: h.trace(inputs[:1] + [(1 << 128) - 1]), -6, "inputs[1] not canonical"),
            (lambda: h.trace(inputs, trace_stride=rows * m - 1, traces=np.zeros((3, rows * m, nl), dtype=np.uint64)), -5, "trace_stride = 5"),
            (lambda: h.trace_dev(d_in.data_ptr(), 3, 1, d_tr.data_ptr(), rows * m - 1, d_out.data_ptr(), s), -5, "trace_stride = 5"),
            (lambda: h.trace_dev(d_in.data_ptr(), 3, 1, d_tr.data_ptr(), big, d_out.data_ptr(), s), -5, "overflows"),
            (lambda: h.hash_dev(d_in.data_ptr(), 1 << 33, 1 << 33, d_out.data_ptr(), s), -5, "overflows"),
            (lambda: h.hash_dev(d_in.data_ptr(), (1 << 40) + 1, 1, d_out.data_ptr(), s), -5, "batch"),
            (lambda: h.hash_dev(0, 3, 1, d_out.data_ptr(), s), -1, "null pointer"),
            (lambda: h.hash_dev(d_in.data_ptr(), 3, 1, 0, s), -1, "null pointer"),
            (lambda: h.trace_dev(d_in.data_ptr(), 3, 1, 0, rows * m, d_out.data_ptr(), s), -1, "null pointer"),
            (lambda: h.hash_dev(d_in.data_ptr() + 8, 3, 1, d_out.data_ptr(), s), -1, "16-byte aligned"),
            (lambda: h.trace_dev(d_in.data_ptr(), 3, 1, d_tr.data_ptr() + 8, rows * m, None, s), -1, "16-byte aligned")):
        refused(fn, code, text)
    assert L.mzk_rescue_hash(None, x.ctypes.data_as(VP), SZ(3), SZ(1), x.ctypes.data_as(VP)) == -1
    assert L.mzk_rescue_hash(h._h, None, SZ(3), SZ(1), x.ctypes.data_as(VP)) == -1
    assert L.mzk_rescue_trace(h._h, x.ctypes.data_as(VP), SZ(3), SZ(1), None, SZ(rows * m), None) == -1
    # nothing to do is not an error, and touches nothing
    assert L.mzk_rescue_hash_dev(h._h, None, SZ(0), SZ(1), None, None) == 0 and L.mzk_rescue_trace_dev(h._h, None, SZ(3), SZ(0), None, SZ(0), None, None) == 0
    assert L.mzk_rescue_hash(h._h, None, SZ(0), SZ(5), None) == 0 and L.mzk_rescue_trace(h._h, None, SZ(5), SZ(0), None, SZ(0), None) == 0
    torch.cuda.synchronize()
    assert (d_out == 7).all() and (d_tr == 7).all(), "a refused call wrote something"
    # the handle still works; the _dev forms take no workspace, and closing the handle leaves the workspace as it was
    h.hash_dev(d_in.data_ptr(), 3, 1, d_out.data_ptr(), s)
    h.trace_dev(d_in.data_ptr(), 3, 1, d_tr.data_ptr(), rows * m, None, s)
    torch.cuda.synchronize()
    assert ints(from_dev(d_out, nl)[:3]) == [rc.model_hash(c, v) for v in inputs]
    h.close()
    h.close()
    assert mz.workspace_bytes() == w0
    assert mz.trim_workspace() >= 0
    with handle(mz, c) as h2:
        assert ints(h2.hash(inputs)) == [rc.model_hash(c, v) for v in inputs]


# ---- preimage -> trace -> proof ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [1, 3])
def test_preimage_to_proof_on_one_stream(env, slots):
    import mpoly_model as mm
    from test_gpu_stark_stages import rescue
    torch, mz, dev = env
    rp, model, air = rescue()                                    # expansion 4, 2 checks
    c = rc.BY_NAME["reference"]
    assert (rp.m, rp.n, rp.alpha, rp.alphainv, rp.mds, rp.rc) == (c["m"], c["n"], c["alpha"], c["alphainv"], c["mds"], c["rc"])
    cons = [mm.terms_of(a) for a in air]
    p, nl, m, rows = rc.M128_P, 2, rp.m, rp.n + 1
    rnd = random.Random(31 + slots)
    inputs = [rc.CHAIN_INPUT, 1, 57322816861100832358702415967512842988][:slots]
    s = torch.cuda.current_stream().cuda_stream
    with mz.Stark(mz.FIELD_M128, 4, 2, m, rows, 2, mm.M128_GEN, cons) as st, handle(mz, c) as h:
        tz_root = st.transition_zerofier_root()
        host_traces = [rp.trace(x) for x in inputs]
        boundaries = [[(0, 1, 0), (rp.n, 0, t[-1][0])] for t in host_traces]
        d = st.dims(boundaries[0])
        rl = d["randomized_trace_length"]
        assert rl > rows
        _, total = mz.stark_proof_layout(mz.FIELD_M128, d)
        random_rows = [[[rnd.randrange(p) for _ in range(m)] for _ in range(rl - rows)] for _ in inputs]
        randomizers = [[rnd.randrange(p) for _ in range(d["randomizer_length"])] for _ in inputs]
        # the proofs from the model's host traces
        want = [st.prove_raw(limbs([v for row in t + rr for v in row], nl).reshape(rl, m, nl), b, limbs(rz, nl))
                for t, rr, b, rz in zip(host_traces, random_rows, boundaries, randomizers)]
        # the trace buffer: every slot rl rows, the random rows already in place behind rows that are still a pattern
        stride = rl * m
        buf = np.full((slots, rl, m, nl), GUARD, dtype=np.uint64)
        for k, rr in enumerate(random_rows):
            buf[k, rows:] = limbs([v for row in rr for v in row], nl).reshape(rl - rows, m, nl)
        d_tr = to_dev(torch, dev, buf)
        d_in = to_dev(torch, dev, limbs(inputs, nl))
        d_rz = [to_dev(torch, dev, limbs(rz, nl)) for rz in randomizers]
        d_proofs = [torch.zeros(total + 8, dtype=torch.uint8, device=dev) for _ in inputs]
        torch.cuda.synchronize()
        h.trace_dev(d_in.data_ptr(), slots, 1, d_tr.data_ptr(), stride, None, s)
        for k in range(slots):                                   # no synchronisation between the trace and the proves
            st.prove_dev(d_tr.data_ptr() + k * stride * 8 * nl, rl, boundaries[k], d_rz[k].data_ptr(), d_proofs[k].data_ptr(), total, s)
        torch.cuda.synchronize()
        for k in range(slots):
            raw = d_proofs[k][:total].cpu().numpy().tobytes()
            assert raw == want[k], "slot %d: the proof from the device trace differs" % k
            proof = mz.stark_unpack_proof(mz.FIELD_M128, d, raw)
            proof.pop("indices")
            assert model.verify(proof, air, boundaries[k], tz_root) is True
        got = from_dev(d_tr, nl).reshape(slots, rl, m, nl)
        assert np.array_equal(got[:, rows:], buf[:, rows:]), "the random rows were written"
