#!/usr/bin/env python3
"""Generate include/mzk_ffi.rs -- the COMPLETE Rust `extern "C"` block for include/mzk.h, one declaration per exported function
(the hand-written block in INTEGRATION.md covered 54 of 98 functions and nothing checked it).

    python tools/gen_rust_ffi.py            # rewrites include/mzk_ffi.rs
    python tools/gen_rust_ffi.py --check    # exit 1 if the committed file is stale

There is no rustc in this image, so the file cannot be compiled here; tests/test_ffi_decls.py parses it back (and the block in
INTEGRATION.md) and compares every name, arity and parameter kind with the C prototypes, which is the mechanical check that is
possible.  The parsing helpers below are shared with that test."""
import os, re, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mzk.h")
OUT = os.path.join(ROOT, "include", "mzk_ffi.rs")

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


def c_structs(path=HDR, names=STRUCTS):
    """[(name, [(field, array length or None)])] for the STRUCTS (or `names`) of the header: `typedef struct X { uint64_t a, b[N], ...; ... } X;` with
    array lengths given as numbers or as the header's enum constants"""
    txt = strip_comments(open(path).read())
    consts = {k: int(v) for body in re.findall(r"enum\s*\{([^}]*)\}", txt) for k, v in re.findall(r"([A-Z][A-Z0-9_]*)\s*=\s*(\d+)", body)}
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


RUST_KEYWORDS = {"in": "input", "type": "kind", "ref": "reference", "use": "use_", "loop": "loop_", "fn": "func", "mod": "modulus", "move": "mv", "box": "box_"}


def emit():
    protos = c_prototypes()
    lines = ['// GENERATED by tools/gen_rust_ffi.py from include/mzk.h -- do not edit; `python tools/gen_rust_ffi.py` rewrites it.',
             '// The complete `extern "C"` surface of libmzk_hip.so (%d functions) for the Rust shim of INTEGRATION.md section 2:' % len(protos),
             '//     #[cfg(feature = "mi355x")] #[path = "../../../../include/mzk_ffi.rs"] pub mod ffi;',
             '// Handles (mzk_srs, mzk_srs_multi, mzk_merkle, mzk_stark, mzk_das_grid, mzk_rescue) are opaque: `c_void` behind the pointer.  Plain structs (%s) are #[repr(C)] below.' % ", ".join(STRUCTS + PLAN_STRUCTS),
             '// Status codes: include/mzk.h.',
             '#![allow(non_camel_case_types, dead_code)]',
             'use std::os::raw::{c_char, c_int, c_uint, c_void};',
             '',
             'pub const MZK_FIELD_FR: c_int = 0;',
             'pub const MZK_FIELD_M128: c_int = 1;',
             'pub const MZK_FIELD_FQ: c_int = 2;',
             'pub const MZK_FIELD_M64: c_int = 3;',
             'pub const MZK_FIELD_M64X3: c_int = 4;',
             'pub const MZK_OK: c_int = 0;',
             'pub const MZK_LAYOUT_CONTIGUOUS: c_int = 0;',
             'pub const MZK_LAYOUT_CYCLIC: c_int = 1;',
             '',
             ] + ['#[repr(C)]\n#[derive(Clone, Copy, Debug)]\npub struct %s {\n%s}\n' % (n, "".join("    pub %s: %s,\n" % (f, "u64" if k is None else "[u64; %d]" % k) for f, k in fs))
                  for n, fs in c_structs(names=STRUCTS + PLAN_STRUCTS)] + [
             '#[link(name = "mzk_hip")]',
             'extern "C" {']
    for name, ret, params in protos:
        ps = ", ".join("%s: %s" % (RUST_KEYWORDS.get(p, p), t) for p, t in params)
        lines.append("    pub fn %s(%s)%s;" % (name, ps, "" if ret is None else " -> " + ret))
    lines.append("}")
    return "\n".join(lines) + "\n"


def rust_decls(text):
    """{name: (ret or None, [types])} for every `pub fn mzk_*` inside a Rust source text (parentheses balanced by hand: a
    callback parameter carries its own `(...) -> c_int`)."""
    text = re.sub(r"/\*.*?\*/", "", re.sub(r"//[^\n]*", "", text), flags=re.S)
    out = {}
    for m in re.finditer(r"pub fn (mzk_[a-z0-9_]+)\s*\(", text):
        i, depth = m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        args = " ".join(text[m.end():i - 1].split())
        tail = text[i:text.index(";", i)]
        ret = tail.split("->", 1)[1] if "->" in tail else None
        types = [" ".join(a.split(":", 1)[1].split()) for a in split_args(args) if a]
        out[m.group(1)] = (None if ret is None else " ".join(ret.split()), types)
    return out


if __name__ == "__main__":
    txt = emit()
    if "--check" in sys.argv:
        ok = os.path.exists(OUT) and open(OUT).read() == txt
        print("include/mzk_ffi.rs is %s" % ("up to date" if ok else "STALE: run python tools/gen_rust_ffi.py"))
        sys.exit(0 if ok else 1)
    open(OUT, "w").write(txt)
    print("wrote %s (%d functions)" % (OUT, len(c_prototypes())))
