"""Every public entry point that takes a field id refuses an id it does not serve with MZK_E_ARG and its own words in
mzk_last_error() -- the id check of each call, pinned call by call: which function names itself how ("ntt: bad field id 7" from the
host-buffer transforms, "ntt: field id 7 has no NTT on this path" from the device ones, "stark_plan: ..." from mzk_stark_new), and that
MZK_FIELD_FQ (2) is as foreign to the Fr / M128 calls as an id that names no field at all (7, -1).

The other arguments are valid and as small as they can be while still reaching the check (one element; two where one would return
early), so a call that let a bad id through would go on to real work instead of failing on something else.  Nothing is launched: the
whole module runs in milliseconds.  It is marked gpu because an entry point initialises the device before it looks at its arguments."""
import ctypes
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_ARG = -1
FQ = 2
FOREIGN = (FQ, 7, -1)         # to the Fr / M128 calls
NO_FIELD = (7, -1)            # to the calls that also serve Fq

SZ = ctypes.c_size_t
CHALLENGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)


class Args:
    """One set of small valid operands, shared by all cases: host buffers (numpy) and device buffers (torch), as void pointers."""

    def __init__(self):
        import torch
        self._keep = []
        self.one = self.host(np.array([1, 0, 0, 0, 1, 0, 0, 0], dtype=np.uint64))        # the element 1, twice (4 limbs each)
        self.out = self.host(np.zeros(64, dtype=np.uint64))
        self.zeros = self.host(np.zeros(64, dtype=np.uint64))                             # offsets {0, 0, ..}, shifts, sign flags
        self.off01 = self.host(np.array([0, 1, 2], dtype=np.uint64))                      # offsets of one-element rows (size_t)
        self.ones_sz = self.host(np.array([1, 1], dtype=np.uint64))                       # lengths (size_t)
        self.exps = self.host(np.array([1, 0], dtype=np.uint32))
        self.probe_in = self.host(np.zeros(64, dtype=np.uint32))
        self.scratch = self.host(np.zeros(256, dtype=np.uint64))                          # handles, lengths, dims: written on success only
        self._dev = torch.zeros(512, dtype=torch.uint8, device="cuda:0")
        self.d_in = ctypes.c_void_p(self._dev.data_ptr())
        self.d_out = ctypes.c_void_p(self._dev.data_ptr() + 256)
        self.d_parts = self.host(np.array([self._dev.data_ptr()], dtype=np.uint64))       # one-entry pointer arrays (mzk_ntt_multi_dev)
        self.d_parts_out = self.host(np.array([self._dev.data_ptr() + 256], dtype=np.uint64))
        self.challenge = CHALLENGE_FN(lambda *a: 1)                                       # never called

    def host(self, a):
        self._keep.append(a)
        return a.ctypes.data_as(ctypes.c_void_p)


def _cases(a):
    """(entry point, arguments after the field id, name in the message, message form, ids).  Built from the sources of the commit before
    the id checks were gathered into one helper: each line is what that function said there."""
    bad, no_ntt = "%s: bad field id %d", "%s: field id %d has no NTT on this path"
    H, O, N = a.one, a.out, None
    c = []

    def add(fn, args, who, form=bad, ids=FOREIGN, fid_at=0):
        c.append((fn, args, who, form, ids, fid_at))

    # transforms, host buffers and device buffers
    add("mzk_ntt", (H, H, O, SZ(1), 0), "ntt")
    add("mzk_ntt_dev", (H, a.d_in, a.d_out, SZ(1), 0, N), "ntt", no_ntt)
    add("mzk_ntt_batch", (H, H, O, SZ(1), SZ(1), 0), "ntt")
    add("mzk_ntt_batch_dev", (H, a.d_in, a.d_out, SZ(1), SZ(1), 0, N), "ntt", no_ntt)       # batch 1 is handed to the single transform
    add("mzk_ntt_batch_dev", (H, a.d_in, a.d_out, SZ(1), SZ(2), 0, N), "ntt", no_ntt)       # batch 2 has its own check
    add("mzk_ntt_columns_dev", (H, a.d_in, a.d_out, SZ(2), SZ(1), 0, N), "ntt_columns", no_ntt)
    add("mzk_ntt_multi", (H, H, O, SZ(1), 0), "ntt_multi", no_ntt)
    add("mzk_ntt_multi_dev", (H, a.d_parts, a.d_parts_out, SZ(1), 0, 0, 0), "ntt_multi", no_ntt)
    add("mzk_coset_lde", (H, SZ(1), H, H, O, SZ(1)), "coset_lde")
    add("mzk_coset_lde_dev", (a.d_in, SZ(1), H, H, a.d_out, SZ(1), N), "coset_lde")
    add("mzk_coset_lde_batch", (H, SZ(1), H, H, O, SZ(1), SZ(1)), "coset_lde")
    add("mzk_coset_lde_batch_dev", (a.d_in, SZ(1), H, H, a.d_out, SZ(1), SZ(1), N), "coset_lde")
    add("mzk_poly_scale", (H, SZ(1), H, N, O), "poly_scale")
    add("mzk_poly_scale_dev", (a.d_in, SZ(1), H, N, a.d_out, N), "poly_scale")
    add("mzk_root_of_unity", (ctypes.c_uint(1), O), "root_of_unity")
    # polynomial arithmetic
    add("mzk_fft_multiply", (H, SZ(1), H, SZ(1), H, O, a.scratch), "fft_multiply")
    add("mzk_fast_multiply", (H, SZ(1), H, SZ(1), H, SZ(2), O, a.scratch), "fast_multiply")
    add("mzk_fast_coset_divide", (H, SZ(1), H, SZ(1), H, H, SZ(2), O, a.scratch), "fast_coset_divide")
    add("mzk_fast_coset_divide_batch_dev", (a.d_in, SZ(1), a.ones_sz, SZ(1), a.d_in, SZ(1), H, H, SZ(2), a.d_out, SZ(1), a.scratch, N), "fast_coset_divide")
    add("mzk_fast_zerofier", (H, SZ(1), H, SZ(2), O, a.scratch), "fast_zerofier")
    add("mzk_fast_evaluate", (H, SZ(1), H, SZ(1), H, SZ(2), O), "fast_evaluate")
    add("mzk_fast_interpolate", (H, H, SZ(1), H, SZ(2), O, a.scratch), "fast_interpolate")
    add("mzk_fast_interpolate_batch", (H, H, SZ(1), SZ(1), H, SZ(2), O, a.scratch), "fast_interpolate")
    add("mzk_fast_interpolate_batch_dev", (H, a.d_in, SZ(1), SZ(1), H, SZ(2), a.d_out, a.scratch, N), "fast_interpolate")
    add("mzk_mpoly_compose_plan", (a.exps, a.off01, SZ(1), SZ(1), a.off01, a.scratch, a.scratch, N), "mpoly_compose")
    add("mzk_mpoly_compose", (H, a.exps, a.off01, SZ(1), SZ(1), H, a.off01, O, SZ(1), a.scratch), "mpoly_compose")
    add("mzk_mpoly_compose_dev", (H, a.exps, a.off01, SZ(1), SZ(1), a.d_in, a.off01, a.d_out, SZ(1), a.scratch, N), "mpoly_compose")
    add("mzk_poly_lincomb", (H, a.off01, SZ(1), H, a.zeros, O, SZ(1), a.scratch), "poly_lincomb")
    add("mzk_poly_lincomb_dev", (a.d_in, a.off01, SZ(1), H, a.zeros, a.d_out, SZ(1), a.scratch, N), "poly_lincomb")
    add("mzk_poly_div_roots", (H, SZ(1), a.ones_sz, SZ(1), H, a.zeros, O, a.scratch), "poly_div_roots")
    add("mzk_poly_div_roots_dev", (a.d_in, SZ(1), a.ones_sz, SZ(1), H, a.zeros, a.d_out, a.scratch, N), "poly_div_roots")
    # FRI and Merkle
    add("mzk_fri_fold", (H, SZ(2), H, H, H, O), "fri_fold")
    add("mzk_fri_fold_dev", (a.d_in, SZ(2), H, H, H, a.d_out, N), "fri_fold")
    add("mzk_merkle_build_field", (H, SZ(1), a.scratch), "merkle")
    add("mzk_merkle_build_field_dev", (a.d_in, SZ(1), a.scratch, N), "merkle")
    add("mzk_merkle_build_field_signed", (H, a.zeros, SZ(1), a.scratch), "merkle")
    add("mzk_merkle_commit_field", (H, SZ(1), O, SZ(48), a.scratch), "merkle")
    add("mzk_merkle_commit_field_dev", (a.d_in, SZ(1), O, SZ(48), a.scratch, N), "merkle")
    add("mzk_merkle_commit_field_signed", (H, a.zeros, SZ(1), O, SZ(48), a.scratch), "merkle")
    add("mzk_merkle_commit_field_batch", (H, SZ(2), SZ(1), O), "merkle")
    add("mzk_merkle_commit_field_batch_dev", (a.d_in, SZ(2), SZ(1), O, N), "merkle")
    commit_tail = (SZ(2), H, H, 1, a.challenge, N, O, a.scratch, O)
    add("mzk_fri_commit", (H,) + commit_tail, "fri_commit")
    add("mzk_fri_commit_signed", (H, a.zeros) + commit_tail, "fri_commit")
    add("mzk_fri_commit_keep_trees", (H, a.zeros) + commit_tail + (a.scratch,), "fri_commit")
    add("mzk_fri_commit_keep_trees_dev", (a.d_in, a.zeros) + commit_tail + (a.scratch,), "fri_commit")
    add("mzk_fri_proof_layout", (SZ(4), SZ(2), SZ(1), a.scratch, N, N, N), "fri_prove")
    add("mzk_fri_prove", (H, N, SZ(4), H, H, SZ(2), SZ(1), O, SZ(512)), "fri_prove")
    add("mzk_fri_prove_dev", (a.d_in, N, SZ(4), H, H, SZ(2), SZ(1), a.d_out, SZ(256), N), "fri_prove")
    # STARK: mzk_stark_new plans first, so it speaks with the plan's name
    plan_head = (SZ(4), SZ(1), SZ(1), SZ(1), SZ(1))
    add("mzk_stark_plan", plan_head + (a.exps, a.off01, SZ(1), a.zeros, a.zeros, SZ(1), a.scratch), "stark_plan")
    add("mzk_stark_new", plan_head + (H, H, a.exps, a.off01, SZ(1), a.scratch), "stark_plan")
    add("mzk_stark_proof_layout", (a.scratch, N, N, a.out), "stark_proof_layout", fid_at=1)
    # calls that serve Fq too: only an id that names no field is refused, each in its own words
    add("mzk_synth_field_dev", (ctypes.c_uint64(1), SZ(1), a.d_out, N), "synth", ids=NO_FIELD)
    add("mzk_selftest_field_asm", (ctypes.c_uint64(1), SZ(1), a.scratch), "selftest", "%s: unknown field id %d", NO_FIELD)
    add("mzk_selftest_field_probe", (0, 0, SZ(1), a.probe_in, O), "field_probe", "%s: no field %d / op 0 / form 0", NO_FIELD)
    add("mzk_host_field_op", (0, H, H, O), "host_field_op", "%s: bad argument", NO_FIELD)
    return c


@pytest.fixture(scope="module")
def args():
    import myzkp_amd as mz
    mz.init(0)
    return Args()


def test_every_field_id_entry_point_is_listed(args):
    """The table above against include/mzk.h: a new entry point with a field_id has to be added here."""
    import os, re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mzk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\bint\s+(mzk_\w+)\s*\([^)]*\bint field_id\b", hdr))
    assert declared == {c[0] for c in _cases(args)}


def test_foreign_field_ids_are_refused_in_each_calls_own_words(args):
    import myzkp_amd as mz
    L = mz.lib()
    failures = []
    for fn, rest, who, form, ids, fid_at in _cases(args):
        for fid in ids:
            argv = list(rest)
            argv.insert(fid_at, ctypes.c_int(fid))
            rc = getattr(L, fn)(*argv)
            msg = L.mzk_last_error().decode()
            want = form % (who, fid) if form.count("%") == 2 else form % who
            if rc != E_ARG or msg != want:
                failures.append("%s(field_id=%d): rc %d, %r; expected %d, %r" % (fn, fid, rc, msg, E_ARG, want))
    assert not failures, "\n".join(failures)
