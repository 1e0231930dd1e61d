"""The evaluation table of a sparse multivariate factor over {0,1}^el (eval_all_binary_combinations of examples/sumcheck's prover;
mzk_mpoly_hypercube_evals) and the host plan of myzkp_amd/csrc/mzk_hypercube_plan.h, restated with Python integers over BN254 Fr.

A factor is a list of terms (coefficient, exponent tuple); a tuple shorter than el is padded with zeros.  Variable i is bit el-1-i of the
table index (BitCombinationsDictOrder), 0^0 = 1.  No GPU, no library."""
import sumcheck_product_model as sm

P = sm.P
TILE_LOG = 10
THREADS = 256
TILE_MAX_GROUPS = 256            # HC_TILE_MAX_GROUPS
TILE_MAX_MASKS = 4096            # HC_TILE_MAX_MASKS
AUTO, TILE, SCATTER = 0, 1, 2


def mask_of(exps, el):
    assert len(exps) <= el
    m = 0
    for i, e in enumerate(exps):
        if e:
            m |= 1 << (el - 1 - i)
    return m


def dense_of(terms, el):
    """the coefficients of the multilinearisation: dense[mask] = sum of the coefficients of the terms with that support"""
    dense = [0] * (1 << el)
    for c, exps in terms:
        m = mask_of(exps, el)
        dense[m] = (dense[m] + c) % P
    return dense


def evals(terms, el):
    """by mask and subset sums: evals[b] = sum of c_t over the terms with mask_t a subset of b"""
    return sm.evals_over_boolean_hypercube(dense_of(terms, el), el)


def evaluate_direct(terms, el, b):
    """MPolynomial.evaluate at the boolean point b, literally: sum_t c_t prod_i pow(b_i, e_t[i]), pow(0, 0) = 1"""
    total = 0
    for c, exps in terms:
        term = c
        for i, e in enumerate(exps):
            term = term * pow((b >> (el - 1 - i)) & 1, e, P)
        total += term
    return total % P


def evals_direct(terms, el, points=None):
    pts = range(1 << el) if points is None else points
    return [evaluate_direct(terms, el, b) for b in pts]


def mle_passes(el):
    n, lo = 0, 0
    while lo < el:
        cb = min(lo, 2)
        lo += min(el - lo, TILE_LOG - cb)
        n += 1
    return n


def plan(factors_exps, el, form=AUTO):
    """hc_plan: factors_exps = per factor the list of exponent tuples.  Term indices are global (factor by factor)."""
    g = min(el, TILE_LOG)
    k = len(factors_exps)
    out = {"g": g, "factors": []}
    t = 0
    for exps in factors_exps:
        by_mask = {}
        for e in exps:
            by_mask.setdefault(mask_of(e, el), []).append(t)
            t += 1
        masks = sorted(by_mask)
        groups = []
        for m in masks:
            if not groups or groups[-1][0] != m >> g:
                groups.append([m >> g, 0])
            groups[-1][1] += 1
        out["factors"].append({"masks": masks, "segments": [by_mask[m] for m in masks], "groups": [tuple(x) for x in groups]})
    out["terms"] = t
    E = sum(len(f["masks"]) for f in out["factors"])
    G = sum(len(f["groups"]) for f in out["factors"])
    out["max_masks"] = max([len(f["masks"]) for f in out["factors"]], default=0)
    out["max_groups"] = max([len(f["groups"]) for f in out["factors"]], default=0)
    out["form"] = form if form != AUTO else (TILE if out["max_groups"] <= TILE_MAX_GROUPS and out["max_masks"] <= TILE_MAX_MASKS else SCATTER)
    out["table_bytes"] = k * 32 << el
    out["mle_passes"] = mle_passes(el)
    if k == 0:
        out.update(launches=0, memsets=0, grid_x=0, grid_y=0, upload_bytes=0, workspace_bytes=0)
        return out
    if out["form"] == TILE:
        out.update(launches=1, memsets=0, grid_x=1 << (el - g), grid_y=k)
        head = (k + 1) + G + (G + 1) + E
    else:
        out.update(launches=1 + k * out["mle_passes"] if E else 0, memsets=1, grid_x=-(-out["max_masks"] // THREADS) if E else 0, grid_y=k if E else 0)
        head = (k + 1) + E
    out["upload_bytes"] = 4 * ((head + 3) // 4 * 4 + 8 * E)
    out["workspace_bytes"] = (out["upload_bytes"] + 255) // 256 * 256
    return out
