"""Entry points called with plain Python values and no ctypes wrapper: a 64-bit seed, a size and device pointers as data_ptr() ints
travel at full width because lib() binds every signature from include/mzk.h (myzkp_amd/_abi.py).  Each result is compared with
the same call made through explicit wrappers, which is right whatever the binding does."""
import ctypes
import numpy as np
import pytest
from orc import FR, M128

pytestmark = pytest.mark.gpu
SEED, N, LOG2 = 2**40 + 3, 257, 10


@pytest.fixture(scope="module")
def env():
    import torch
    import myzkp_amd as mz
    mz.init(0)
    return torch, mz, mz.lib(), torch.cuda.current_stream().cuda_stream


def _host(t, nl):
    return t.cpu().numpy().view(np.uint64).reshape(-1, nl)


@pytest.mark.parametrize("fid", [FR, M128])
def test_seed_size_and_pointers_as_plain_ints(env, fid):
    torch, mz, L, st = env
    nl = mz.LIMBS[fid]
    plain, wrapped, low = (torch.zeros(N * nl, dtype=torch.int64, device="cuda") for _ in range(3))
    assert L.mzk_synth_field_dev(fid, SEED, N, plain.data_ptr(), st) == 0
    assert L.mzk_synth_field_dev(fid, ctypes.c_uint64(SEED), ctypes.c_size_t(N), ctypes.c_void_p(wrapped.data_ptr()), ctypes.c_void_p(st)) == 0
    assert L.mzk_synth_field_dev(fid, SEED % 2**32, N, low.data_ptr(), st) == 0      # what a seed cut to 32 bits would give
    torch.cuda.synchronize()
    assert plain.data_ptr() >= 2**32                 # the pointers are of the kind that a C int would cut
    assert torch.equal(plain, wrapped) and not torch.equal(plain, low)

    n = 1 << LOG2
    x, out = torch.zeros(n * nl, dtype=torch.int64, device="cuda"), torch.zeros(n * nl, dtype=torch.int64, device="cuda")
    w = mz.root_of_unity(fid, LOG2)
    root = mz.to_limbs([w], nl)
    assert L.mzk_synth_field_dev(fid, SEED, n, x.data_ptr(), st) == 0
    assert L.mzk_ntt_dev(fid, root.ctypes.data, x.data_ptr(), out.data_ptr(), n, 0, st) == 0, L.mzk_last_error().decode()
    torch.cuda.synchronize()
    assert np.array_equal(_host(out, nl), mz.ntt(fid, w, _host(x, nl)))


def test_a_pointer_return_needs_no_restype_from_the_caller(env):
    torch, mz, L, st = env
    # the reference: the prototype stated by hand, on a second handle of the same library that nothing has bound
    by_hand = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_int)(("mzk_ctx_stream", ctypes.CDLL(mz._lib.SO)))
    want = by_hand(0)
    assert want and L.mzk_ctx_stream(0) == want
