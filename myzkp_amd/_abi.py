"""The one reader of include/mzk.h: its prototypes, structs and enum constants, and the ctypes signatures that follow from them.

A prototype is read into Rust spelling (`c_int`, `usize`, `u64`, `*const T`, `*mut T`, None for void): tools/gen_rust_ffi.py prints that form
as include/mzk_ffi.rs, and signatures() / bind() map the same form onto ctypes, so that `lib().mzk_x(n, ptr, seed)` takes plain Python
values at their full width.  A new entry point needs its prototype in the header and nothing here.  No torch, no numpy, no library."""
import ctypes, os, re

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mzk.h")

HANDLES = ("mzk_srs_multi", "mzk_srs", "mzk_merkle", "mzk_stark", "mzk_das_grid", "mzk_rescue")
STRUCTS = ("mzk_stark_dims",)           # plain structs of uint64_t fields, passed by pointer: emitted as #[repr(C)] (c_structs)
PLAN_STRUCTS = ("mzk_hypercube_plan",)   # the same kind of struct, added later: c_structs() keeps answering for STRUCTS alone
SCALARS = {"int": "c_int", "unsigned": "c_uint", "unsigned int": "c_uint", "size_t": "usize", "uint64_t": "u64", "uint32_t": "u32",
           "uint8_t": "u8", "double": "f64", "char": "c_char", "void": "c_void"}
CHALLENGE = 'extern "C" fn(*mut c_void, c_int, c_int, *const u8, usize, *mut u64) -> c_int'
SUMCHECK_CHALLENGE = 'extern "C" fn(*mut c_void, c_int, *const u64, *mut u64) -> c_int'   # mzk_sumcheck_challenge_fn (g is NULL for beta)
CALLBACKS = {"mzk_fri_challenge_fn": CHALLENGE, "mzk_sumcheck_challenge_fn": SUMCHECK_CHALLENGE}


def strip_comments(txt):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def c_prototypes(path=HDR):
    """[(name, return type in Rust spelling or None for void, [(param name, Rust type)])] in header order."""
    txt = strip_comments(open(path).read())
    txt = txt[txt.index('extern "C" {') + len('extern "C" {'):]
    protos = []
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(mzk_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", txt, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        if ret.startswith("typedef"):
            continue
        params = []
        if args and args != "void":
            for i, a in enumerate(split_args(args)):
                pname, ptype = c_param(a, i)
                params.append((pname, ptype))
        protos.append((name, None if ret == "void" else c_type(ret), params))
    return protos


def enum_blocks(path=HDR):
    """[{NAME: integer}] for every `enum { ... }` of the header, in header order"""
    txt = strip_comments(open(path).read())
    return [{k: int(v) for k, v in re.findall(r"([A-Z][A-Z0-9_]*)\s*=\s*(-?\d+)", body)} for body in re.findall(r"enum\s*\{([^}]*)\}", txt)]


def constants(path=HDR):
    """{NAME: integer} over every enum of the header"""
    return {k: v for block in enum_blocks(path) for k, v in block.items()}


def index_names(count_name, path=HDR):
    """The lower-case names of an index enum in index order: the members of the enum that declares `count_name` (MZK_FRI_SECTIONS,
    MZK_DAS_PLAN_WORDS) whose value is below it, without the prefix they share with it -- MZK_FRI_TOP_INDICES = 1 is "top_indices"."""
    block = next(b for b in enum_blocks(path) if count_name in b)
    prefix = count_name[:count_name.rindex("_") + 1]
    names = sorted((v, k) for k, v in block.items() if 0 <= v < block[count_name] and k != count_name)
    assert [v for v, _ in names] == list(range(block[count_name])) and all(k.startswith(prefix) for _, k in names), count_name
    return tuple(k[len(prefix):].lower() for _, k in names)


def c_structs(path=HDR, names=STRUCTS):
    """[(name, [(field, array length or None)])] for the STRUCTS (or `names`) of the header: `typedef struct X { uint64_t a, b[N], ...; ... } X;` with
    array lengths given as numbers or as the header's enum constants"""
    txt = strip_comments(open(path).read())
    consts = constants(path)
    out = []
    for name in names:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            assert decl.startswith("uint64_t "), decl
            for f in decl[len("uint64_t "):].split(","):
                m = re.match(r"\s*([a-z_0-9]+)\s*(?:\[([A-Za-z0-9_]+)\])?\s*$", f)
                n = m.group(2)
                fields.append((m.group(1), None if n is None else (int(n) if n.isdigit() else consts[n])))
        out.append((name, fields))
    return out


def split_args(args):
    out, depth, cur = [], 0, ""
    for ch in args:
        if ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip()); cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def c_param(a, idx):
    a = a.strip()
    for cb, rust in CALLBACKS.items():
        if a.startswith(cb):
            return (a.split()[-1], rust)
    m = re.match(r"(.*?)([A-Za-z_][A-Za-z0-9_]*)\s*(\[[0-9]*\])?$", a)
    ctype, name, arr = m.group(1).strip(), m.group(2), m.group(3)
    if not ctype:                    # unnamed parameter
        ctype, name = a, "arg%d" % idx
    if arr:
        ctype += "*"
    return (name, c_type(ctype))


def c_type(t):
    """C declarator (without the name) -> Rust type.  Pointers are read right to left; `const` binds to what is left of it."""
    t = t.replace("*", " * ")
    toks = t.split()
    # base: everything up to the first '*'
    k = toks.index("*") if "*" in toks else len(toks)
    base = [x for x in toks[:k] if x != "const"]
    base_const = "const" in toks[:k]
    bname = " ".join(base)
    if bname in HANDLES or bname.startswith("struct "):
        rust = "c_void"
    elif bname in STRUCTS or bname in PLAN_STRUCTS:
        rust = bname
    elif bname in SCALARS:
        rust = SCALARS[bname]
    else:
        raise ValueError("unknown C type %r in %r" % (bname, t))
    rest = toks[k:]
    pointee_const = base_const
    i = 0
    while i < len(rest):
        assert rest[i] == "*", rest
        rust = ("*const " if pointee_const else "*mut ") + rust
        pointee_const = False
        i += 1
        if i < len(rest) and rest[i] == "const":
            pointee_const = True
            i += 1
    return rust


# ---- ctypes ------------------------------------------------------------------------------------------------------------------------------
_BY_VALUE = {"c_int": ctypes.c_int, "c_uint": ctypes.c_uint, "usize": ctypes.c_size_t, "u64": ctypes.c_uint64, "u32": ctypes.c_uint32}
_RETURNS = dict(_BY_VALUE, **{"*const c_char": ctypes.c_char_p, "*mut c_void": ctypes.c_void_p})


def _argtype(rust):
    """every pointer -- handle, T**, struct, string, callback -- is c_void_p: it takes None, an int, byref(), arrays, bytes and CFUNCTYPE
    instances, which is what the callers pass"""
    if rust.startswith("*") or rust.startswith('extern "C" fn'):
        return ctypes.c_void_p
    if rust not in _BY_VALUE:
        raise ValueError("no ctypes class for a %r parameter" % rust)
    return _BY_VALUE[rust]


def _restype(rust):
    if rust is not None and rust not in _RETURNS:
        raise ValueError("no ctypes class for a %r return" % rust)
    return None if rust is None else _RETURNS[rust]


def signatures(path=HDR):
    """{name: (restype, [argtypes])} for every prototype of the header; a type without a ctypes class raises"""
    return {name: (_restype(ret), [_argtype(t) for _, t in params]) for name, ret, params in c_prototypes(path)}


def bind(cdll, path=HDR):
    """Set argtypes and restype on every function of the header that `cdll` exports (a build may lack some; what the header does not
    declare is left alone)."""
    for name, (restype, argtypes) in signatures(path).items():
        fn = getattr(cdll, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return cdll
