"""The ctypes signatures that myzkp_amd/_abi.py binds from include/mzk.h: every prototype gets one, every by-value parameter its own
width, and a value that does not fit in 32 bits comes back whole through a real call -- made on a six-function echo library
(tests/hostcheck/abi_echo.h / .cpp) read and bound by the same code.  CPU only."""
import ctypes, os, subprocess
import pytest
import myzkp_amd
from myzkp_amd import _abi, _lib as mzlib

HERE = os.path.dirname(os.path.abspath(__file__))
ECHO_H = os.path.join(HERE, "hostcheck", "abi_echo.h")
BY_VALUE = {"c_int": ctypes.c_int, "c_uint": ctypes.c_uint, "usize": ctypes.c_size_t, "u64": ctypes.c_uint64, "u32": ctypes.c_uint32}
WIDE = (2**32 + 5, 2**63 + 1, 2**64 - 1)
ADDRESS = 0x7f123456789a


def test_every_prototype_has_a_signature_of_its_own_arity_and_widths():
    sigs = _abi.signatures()
    protos = _abi.c_prototypes()
    assert sorted(sigs) == sorted(myzkp_amd.DECLARED_SYMBOLS) and len(sigs) == len(protos) >= 190
    by_value = dict.fromkeys(BY_VALUE, 0)
    for name, ret, params in protos:
        restype, argtypes = sigs[name]
        assert len(argtypes) == len(params), name
        for (pname, rust), got in zip(params, argtypes):
            assert got is not None, (name, pname)
            if rust in BY_VALUE:
                assert got is BY_VALUE[rust], (name, pname)
                by_value[rust] += 1
            else:
                assert (rust.startswith("*") or rust.startswith('extern "C" fn')) and got is ctypes.c_void_p, (name, pname, rust)
        assert restype is {None: None, "c_int": ctypes.c_int, "usize": ctypes.c_size_t, "*const c_char": ctypes.c_char_p,
                           "*mut c_void": ctypes.c_void_p}[ret], name
    assert all(by_value.values()), by_value             # the header has parameters of each of the five kinds
    other = {name: sigs[name][0] for name, ret, _ in protos if ret != "c_int"}
    assert len(other) == 15
    assert {n for n, t in other.items() if t is ctypes.c_size_t} == {"mzk_srs_len", "mzk_srs_table_bytes", "mzk_srs_multi_shard_lo"}
    assert {n for n, t in other.items() if t is ctypes.c_char_p} == {"mzk_last_error", "mzk_prof_name"}
    assert {n for n, t in other.items() if t is ctypes.c_void_p} == {"mzk_ctx_stream"}
    assert sum(t is None for t in other.values()) == 9


def test_a_type_without_a_ctypes_class_is_an_error(tmp_path):
    hdr = tmp_path / "bad.h"
    hdr.write_text('extern "C" {\nint mzk_takes_double(double x);\n}\n')
    with pytest.raises(ValueError, match="f64"):
        _abi.signatures(str(hdr))
    hdr.write_text('extern "C" {\ndouble mzk_returns_double(int x);\n}\n')
    with pytest.raises(ValueError, match="f64"):
        _abi.signatures(str(hdr))


@pytest.fixture(scope="module")
def echo_so(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("abi_echo") / "libabi_echo.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(HERE, "hostcheck", "abi_echo.cpp")])
    return so


def test_wide_values_round_trip_through_a_bound_library(echo_so):
    assert sorted(_abi.signatures(ECHO_H)) == ["mzk_echo_handle", "mzk_echo_mixed", "mzk_echo_name", "mzk_echo_ptr", "mzk_echo_u64", "mzk_echo_usize"]
    L = _abi.bind(ctypes.CDLL(echo_so), ECHO_H)
    out, back = ctypes.c_uint64(), ctypes.c_size_t()
    for v in WIDE:
        assert L.mzk_echo_usize(v) == v
        assert L.mzk_echo_u64(v, ctypes.byref(out)) == 0 and out.value == v
    assert L.mzk_echo_ptr(ADDRESS, ctypes.byref(back)) == 0 and back.value == ADDRESS
    assert L.mzk_echo_ptr(None, ctypes.byref(back)) == 0 and back.value == 0
    assert L.mzk_echo_handle(ADDRESS) == ADDRESS and L.mzk_echo_handle(None) is None
    assert L.mzk_echo_name(0) == b"zero" and L.mzk_echo_name(1) == b"one"
    five = (ctypes.c_uint64 * 5)()
    assert L.mzk_echo_mixed(-3, WIDE[0], 2**32 - 1, WIDE[2], ADDRESS, five) == -3
    assert list(five) == [2**64 - 3, WIDE[0], 2**32 - 1, WIDE[2], ADDRESS]
    # the forms the callers already use keep working
    buf = (ctypes.c_uint8 * 4)()
    assert L.mzk_echo_handle(buf) == ctypes.addressof(buf) == L.mzk_echo_handle(ctypes.c_void_p(ctypes.addressof(buf)))
    assert L.mzk_echo_usize(ctypes.c_size_t(WIDE[1])) == WIDE[1] == L.mzk_echo_usize(ctypes.c_uint64(WIDE[1]))
    # ... and a value of the wrong kind is refused, not reinterpreted
    for wrong in (ctypes.c_int(1), 1.0):
        with pytest.raises(ctypes.ArgumentError):
            L.mzk_echo_usize(wrong)


def test_the_same_calls_unbound_lose_the_upper_half(echo_so):
    """what bind() is for: without argtypes a plain int travels as a C int"""
    U = ctypes.CDLL(echo_so)
    out = ctypes.c_uint64()
    U.mzk_echo_u64(WIDE[0], ctypes.byref(out))
    assert out.value == 5
    assert U.mzk_echo_usize(WIDE[0]) == 5


def test_bind_skips_what_a_build_lacks_and_leaves_the_undeclared_alone(echo_so, tmp_path):
    L = ctypes.CDLL(echo_so)
    unbound = (L.mzk_echo_handle.restype, L.mzk_echo_handle.argtypes)
    hdr_one = tmp_path / "one.h"
    hdr_one.write_text('extern "C" {\nsize_t mzk_echo_usize(size_t v);\nsize_t mzk_echo_absent(size_t v);\n}\n')
    assert sorted(_abi.signatures(str(hdr_one))) == ["mzk_echo_absent", "mzk_echo_usize"]
    _abi.bind(L, str(hdr_one))
    assert L.mzk_echo_usize(WIDE[0]) == WIDE[0]
    assert (L.mzk_echo_handle.restype, L.mzk_echo_handle.argtypes) == unbound


def test_structs_and_constants_come_from_the_header():
    consts = _abi.constants()
    for cls, name in ((myzkp_amd.StarkDims, "mzk_stark_dims"), (mzlib._HypercubePlan, "mzk_hypercube_plan")):
        (got_name, fields), = _abi.c_structs(names=(name,))
        assert got_name == name
        assert [(f, None if t is ctypes.c_uint64 else t._length_) for f, t in cls._fields_] == fields
        assert all(t is ctypes.c_uint64 or t._type_ is ctypes.c_uint64 for _, t in cls._fields_)
        assert ctypes.sizeof(cls) == 8 * sum(k or 1 for _, k in fields)
    L = mzlib
    assert L.ERRORS[0] == "MZK_OK" and L.ERRORS[-1] == "MZK_E_ARG" and L.ERRORS[-12] == "MZK_E_NOMEM"
    for code, name in L.ERRORS.items():
        assert consts[name] == code
    assert (L.FIELD_FR, L.FIELD_M128, L.FIELD_FQ, L.FIELD_M64, L.FIELD_M64X3) == (0, 1, 2, 3, 4)
    for names, count in ((L.SCP_SECTIONS, "MZK_SCP_SECTIONS"), (L.FRI_SECTIONS, "MZK_FRI_SECTIONS"), (L.STARK_SECTIONS, "MZK_STARK_SECTIONS"),
                         (L.DAS_PLAN_FIELDS, "MZK_DAS_PLAN_WORDS"), (L.RESCUE_PLAN_FIELDS, "MZK_RESCUE_PLAN_WORDS")):
        prefix = count[:count.rindex("_") + 1]
        assert len(names) == consts[count] and [consts[prefix + n.upper()] for n in names] == list(range(len(names)))
