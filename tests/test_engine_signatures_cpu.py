"""CPU: cofhe_amd.engine's signature table against include/cofhe_hip.h, prototype by prototype, and against what
load_library() installed on the library; plain Python integers beyond 32 bits reach the C side whole.  No kernel runs."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

PARAM_CLASS = {"uint32_t": "u", "uint64_t": "q", "size_t": "z", "int": "i", "int64_t": "l"}       # "p": anything with * or [
RETURN_CLASS = {"int": "i", "void": "v", "size_t": "z", "const char *": "s"}
CTYPE = {"p": C.c_void_p, "u": C.c_uint32, "q": C.c_uint64, "z": C.c_size_t, "i": C.c_int, "l": C.c_int64,
         "v": None, "s": C.c_char_p}


def _param_class(text):
    if "*" in text or "[" in text:
        return "p"
    words = [w for w in text.split() if w != "const"]
    assert len(words) == 2 and words[0] in PARAM_CLASS, "a parameter of a new kind: %r" % text       # type and name
    return PARAM_CLASS[words[0]]


def header_prototypes():
    """{name: "r:params"} of every prototype of the header, in the table's spelling"""
    text = open(os.path.join(ROOT, "include", "cofhe_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", text, flags=re.M)
    protos = {}
    for stmt in re.split(r"[;{}]", text):
        if "(" not in stmt:
            continue                                                     # a struct member, a typedef, extern "C"
        m = re.fullmatch(r"\s*(.*?)\s*\b(cofhe_hip_\w+)\s*\(([^()]*)\)\s*", stmt, flags=re.S)
        assert m, "not a prototype: %r" % stmt
        ret, name, params = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        assert ret in RETURN_CLASS, "a return type of a new kind: %r %s" % (ret, name)
        assert name not in protos, name
        plist = [] if params in ("void", "") else params.split(",")
        protos[name] = RETURN_CLASS[ret] + ":" + "".join(_param_class(p) for p in plist)
    return protos


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cofhe_amd import load_library
    return load_library()


@pytest.fixture(scope="module")
def host_engine(lib):
    from cofhe_amd.engine import Engine
    eng = Engine.__new__(Engine)          # host-only methods need no GPU context
    eng.L = lib
    return eng


def test_the_parser_finds_the_header():
    protos = header_prototypes()
    assert len(protos) >= 100
    assert protos["cofhe_hip_last_error"] == "s:" and protos["cofhe_hip_ctx_destroy"] == "v:p"
    assert protos["cofhe_hip_packed_size_bound"] == "z:qiu" and protos["cofhe_hip_ctx_set_option"] == "i:ppl"
    assert protos["cofhe_hip_ctx_create"] == "i:ipzp"


def test_table_names_are_the_headers():
    from cofhe_amd import engine
    protos = header_prototypes()
    assert sorted(set(engine.SIGNATURES) - set(protos)) == []
    assert sorted(set(protos) - set(engine.SIGNATURES)) == []


def test_table_entries_are_the_headers():
    from cofhe_amd import engine
    protos = header_prototypes()
    for name in sorted(protos):
        want_ret, want_params = protos[name].split(":")
        got_ret, got_params = engine.SIGNATURES[name].split(":")
        assert got_ret == want_ret, name
        assert len(got_params) == len(want_params), name
        for i, (g, w) in enumerate(zip(got_params, want_params)):
            assert g == w, "%s: parameter %d" % (name, i)


def test_the_loaded_library_carries_the_table(lib):
    from cofhe_amd import engine
    for name, sig in engine.SIGNATURES.items():
        ret, params = sig.split(":")
        fn = getattr(lib, name)
        assert fn.restype is CTYPE[ret], name
        assert list(fn.argtypes) == [CTYPE[p] for p in params], name


def test_plain_64_bit_integers_survive(lib, host_engine):
    from cofhe_amd import shard
    n = 2 ** 33 + 5
    for world in (1, 3):
        want = shard.row_partition(n, world)
        for rank in range(world):
            r0, nl = host_engine.shard_rows(n, world, rank)
            assert (r0, r0 + nl) == want[rank], (world, rank)
    assert host_engine.packed_size_bound(2 ** 33, 2, 1) == lib.cofhe_hip_packed_size_bound(C.c_uint64(2 ** 33), C.c_int(2), C.c_uint32(1))
    assert host_engine.packed_size_bound(2 ** 33, 2, 1) > 2 ** 33


def test_a_short_host_record_is_refused():
    import numpy as np
    from cofhe_amd import engine
    with pytest.raises(AssertionError):
        engine._host_record(np.zeros(engine.REC_WORDS - 1, dtype=np.uint32))
    with pytest.raises(AssertionError):
        engine._host_record(np.zeros(engine.EXP_REC_WORDS - 1, dtype=np.uint32), engine.EXP_REC_WORDS)
    rec = engine._host_record(list(range(engine.REC_WORDS)))
    assert rec.dtype == np.uint32 and rec.flags["C_CONTIGUOUS"] and rec.size == engine.REC_WORDS
