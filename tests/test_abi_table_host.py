"""CPU: the binding's ABI table (phl._ABI) is include/phl.h, prototype for prototype; load_library() applies it to
every exported function; and nothing else in the Python sources declares a signature of the library."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C type -> the table's code (phl/__init__.py: _KINDS); anything with '*' or '[' is a pointer
ARG_KINDS = {"phl_stream": "S", "int": "i", "int64_t": "q", "unsigned": "I", "uint64_t": "Q", "float": "f", "double": "d"}
RET_KINDS = {"int": "i", "int64_t": "q", "size_t": "N", "const char *": "z"}


def _stripped_header():
    text = open(os.path.join(ROOT, "include", "phl.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return "\n".join(line for line in text.split("\n") if not line.lstrip().startswith("#"))


def _arg_kind(arg):
    if "*" in arg or "[" in arg:
        return "P"
    words = arg.split()
    assert len(words) == 2, f"argument {arg!r} is not 'type name'"
    return ARG_KINDS[words[0]]


def _header_table():
    """[(name, return kind, argument kinds)] of every prototype, in the header's order."""
    text = _stripped_header()
    protos = re.findall(r"([A-Za-z_][\w\s\*]*?)\b(phl_\w+)\s*\(([^()]*)\)\s*;", text)
    # every declaration that ends in ';' was read: a prototype the pattern above cannot parse fails here, it is not skipped
    assert len(protos) >= len(re.findall(r"phl_\w+\s*\([^;{}]*;", text)) >= 75
    table = []
    for ret, name, args in protos:
        args = " ".join(args.split())
        kinds = "" if args == "void" else "".join(_arg_kind(a.strip()) for a in args.split(","))
        table.append((name, RET_KINDS[" ".join(ret.split())], kinds))
    return table


def test_table_equals_header():
    import phl

    header, table = _header_table(), [tuple(row) for row in phl._ABI]
    assert len({name for name, _, _ in table}) == len(table), "a name is listed twice"
    assert [name for name, _, _ in table] == [name for name, _, _ in header]        # no extra, no missing, header's order
    for got, want in zip(table, header):
        assert got == want, f"{got[0]}: the table says {got[1:]}, include/phl.h says {want[1:]}"
    assert set("".join(args for _, _, args in table)) == set("PSiqIQfd")
    assert {ret for _, ret, _ in table} == set("iqNz")
    assert set(phl._KINDS) == set("PSiqIQfd") | set("iqNz")
    sizes = {"P": ctypes.sizeof(ctypes.c_void_p), "S": ctypes.sizeof(ctypes.c_void_p), "i": 4, "q": 8, "I": 4, "Q": 8, "f": 4,
             "d": 8, "N": ctypes.sizeof(ctypes.c_size_t), "z": ctypes.sizeof(ctypes.c_char_p)}
    assert {k: ctypes.sizeof(t) for k, t in phl._KINDS.items()} == sizes
    assert phl._KINDS["f"] is ctypes.c_float and phl._KINDS["d"] is ctypes.c_double
    assert phl._KINDS["I"] is ctypes.c_uint and phl._KINDS["Q"] is ctypes.c_uint64


def test_load_applies_the_table():
    import phl

    if not os.path.exists(phl.LIB_PATH):
        pytest.skip("libphl.so is not built")
    lib = phl.load_library()
    seen = 0
    for name, ret, args in phl._ABI:
        if not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        assert fn.restype is phl._KINDS[ret], name
        assert fn.argtypes is not None and list(fn.argtypes) == [phl._KINDS[k] for k in args], name
        seen += 1
    assert seen >= 70


def test_no_second_declaration_site():
    """Only the table loop of load_library() assigns .argtypes / .restype of a library function."""
    files = [os.path.join(ROOT, "bench.py")]
    for top in ("depth-estimation_amd", "tools", "examples"):
        for folder, _, names in os.walk(os.path.join(ROOT, top)):
            files += [os.path.join(folder, n) for n in names if n.endswith(".py")]
    assert len(files) > 10
    sites = []
    for path in files:
        for no, line in enumerate(open(path, encoding="utf-8", errors="replace"), 1):
            if re.search(r"\.(argtypes|restype)\b[^=]*=(?!=)", line):
                sites.append(f"{os.path.relpath(path, ROOT)}:{no}: {line.strip()}")
    assert len(sites) == 1 and "fn.restype, fn.argtypes = " in sites[0] and sites[0].startswith(
        os.path.join("depth-estimation_amd", "phl", "__init__.py")), sites
