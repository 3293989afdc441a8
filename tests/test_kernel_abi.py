"""The ctypes signature table of libpha_kernels.so (ops/_abi.py) against the C sources it describes.

Source text only: no built library, no GPU. Every ``PHA_API`` prototype in csrc/kernels/*.hip must
have exactly one table entry with the same return type and the same argument types in order, every
``.pha_*`` attribute the Python bindings use must be a table entry, and no binding module declares
argument types of its own. A wrong type at this boundary hands a kernel a truncated stride or
pointer, so a new entry point fails here until its line in the table is right.
"""
import glob
import os
import re
from ctypes import c_float, c_int, c_long, c_uint, c_void_p

from paddle_hackathon_amd.ops import _abi

PKG = os.path.dirname(os.path.dirname(os.path.abspath(_abi.__file__)))
CODES = {c_int: "I", c_long: "LG", c_float: "F", c_uint: "U", c_void_p: "P"}
SCALARS = {"int": "I", "long": "LG", "float": "F", "unsigned": "U", "hipStream_t": "P"}
PROTO = re.compile(r"\bPHA_API\s+([\w\s*]+?)\s*\b(pha_\w+)\s*\(([^)]*)\)")


def _code(decl, named):
    """C parameter declaration (or return type, ``named`` False) -> table code; unknown types raise"""
    decl = decl.split("=")[0].strip()
    if "*" in decl:
        return "P"
    toks = [t for t in decl.split() if t != "const"]
    ctype = " ".join(toks[:-1] if named and len(toks) > 1 else toks)
    if ctype not in SCALARS:
        raise AssertionError(f"type {ctype!r} in {decl!r}: not one the signature table can express")
    return SCALARS[ctype]


def _prototypes():
    """name -> (return code, [argument codes], file) of every PHA_API function in the kernel sources"""
    protos = {}
    files = sorted(glob.glob(os.path.join(PKG, "csrc", "kernels", "*.hip")))
    assert files, "no kernel sources found"
    for path in files:
        with open(path) as f:
            src = f.read()
        src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
        src = re.sub(r"//[^\n]*", " ", src)
        for ret, name, params in PROTO.findall(src):
            assert name not in protos, f"{name} is defined in {protos[name][2]} and {os.path.basename(path)}"
            params = params.strip()
            args = [] if params in ("", "void") else [_code(p, True) for p in params.split(",")]
            protos[name] = (_code(ret, False), args, os.path.basename(path))
    return protos


def _binding_sources():
    files = sorted(glob.glob(os.path.join(PKG, "ops", "*.py"))) + [os.path.join(PKG, "parallel", "ps", "gpu_ps.py")]
    for path in files:
        with open(path) as f:
            yield os.path.relpath(path, PKG), f.read()


def test_table_names_match_the_sources():
    protos, table = _prototypes(), _abi.SIGNATURES
    assert len(protos) > 80, f"only {len(protos)} prototypes parsed: the pattern no longer fits the sources"
    undeclared = sorted(set(protos) - set(table))
    stale = sorted(set(table) - set(protos))
    assert not undeclared, f"exported by the kernel sources but missing from ops/_abi.py: {undeclared}"
    assert not stale, f"in ops/_abi.py but exported by no kernel source: {stale}"


def test_table_signatures_match_the_prototypes():
    protos = _prototypes()
    wrong = []
    for name, (restype, argtypes) in _abi.SIGNATURES.items():
        if name not in protos:
            continue   # reported by test_table_names_match_the_sources
        ret, args, path = protos[name]
        have = [CODES[t] for t in argtypes]
        if CODES[restype] != ret:
            wrong.append(f"{name} ({path}): returns {ret}, table says {CODES[restype]}")
        if len(have) != len(args):
            wrong.append(f"{name} ({path}): {len(args)} parameters, table has {len(have)}")
            continue
        wrong += [f"{name} ({path}): parameter {i} is {c}, table says {h}"
                  for i, (c, h) in enumerate(zip(args, have)) if c != h]
    assert not wrong, "\n".join(wrong)


def test_bindings_call_only_declared_entry_points():
    used = {}
    for rel, src in _binding_sources():
        for name in re.findall(r"\.(pha_\w+)", src):
            used.setdefault(name, rel)
    assert used, "no .pha_* call found in the binding modules"
    unknown = {n: rel for n, rel in used.items() if n not in _abi.SIGNATURES}
    assert not unknown, f"called without a signature in ops/_abi.py: {unknown}"


def test_no_signature_is_declared_outside_the_table():
    stray = []
    for rel, src in _binding_sources():
        if rel == os.path.join("ops", "_abi.py"):
            continue
        for no, line in enumerate(src.split("\n"), 1):
            # the HIP runtime's own functions (hipHostMalloc, hipMemcpyAsync) are not this library's
            if re.search(r"\b(argtypes|restype)\b[^=]*=(?!=)", line) and not re.search(r"\.hip[A-Z]\w*\.", line):
                stray.append(f"{rel}:{no}: {line.strip()}")
    assert not stray, "ctypes signatures belong in ops/_abi.py:\n" + "\n".join(stray)
