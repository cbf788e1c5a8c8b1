"""_lib.ABI and the ctypes structures held to include/lva_decoder.h, without a GPU: the header is parsed (comments stripped,
continuation lines joined) and every prototype and every structure compared with what the Python layer declares.  An
argtypes list that is one entry short, or a 32-bit slot where the header has 64 bits, still loads and mostly still runs;
here it fails."""
import ctypes
import os
import re

import pytest

from nanopore_dna_storage_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C scalar type -> (bytes, signed, floating); `char` by value does not occur in the header
SCALARS = {"int": (4, True, False), "int32_t": (4, True, False), "uint32_t": (4, False, False), "int64_t": (8, True, False),
           "uint64_t": (8, False, False), "uint16_t": (2, False, False), "uint8_t": (1, False, False), "double": (8, False, True),
           "float": (4, False, True)}
# header structure -> Python class
STRUCTS = {"lva_config": _lib.Config, "lva_code_info": _lib.CodeInfoStruct, "lva_profile": _lib.Profile,
           "lva_payload_pos": _lib.PayloadPos, "lva_experiment_barcodes": _lib.ExperimentBarcodes, "lva_demux_pos": _lib.DemuxPos,
           "lva_list_stat": _lib.ListStat, "lva_kernel_plan_info": _lib.KernelPlanInfo}


def _header():
    with open(os.path.join(ROOT, "include", "lva_decoder.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = text.replace("\\\n", " ")
    text = "\n".join(ln for ln in text.split("\n") if not ln.lstrip().startswith("#"))     # preprocessor lines
    return re.sub(r"\s+", " ", text)                                                        # prototypes span lines


def _ctype_class(t):
    """a ctypes type -> "ptr", or (bytes, signed, floating) of a scalar"""
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "ptr"
    assert issubclass(t, ctypes._SimpleCData), t
    code = t._type_
    return (ctypes.sizeof(t), code in "bhilq", code in "fd")


def _c_class(decl):
    """the type part of a C declaration (no name) -> "ptr", or (bytes, signed, floating)"""
    if "*" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    assert len(words) == 1 and words[0] in SCALARS, decl
    return SCALARS[words[0]]


def _split_param(p):
    """'const float *post' -> ('const float *', 'post')"""
    m = re.match(r"^(.*?)(\w+)$", p.strip())
    assert m and m.group(1).strip(), p
    return m.group(1).strip(), m.group(2)


def prototypes():
    """{name: (return type text, [parameter type text])} of every function the header declares"""
    out = {}
    for ret, name, params in re.findall(r"(?<=[;}])\s*((?:const\s+)?\w+\s*\**)\s*\b(lva_\w+)\s*\(([^()]*)\)\s*;", _header()):
        assert name not in out, name
        params = params.strip()
        out[name] = (ret.replace(" ", ""), [] if params == "void" else [_split_param(p)[0] for p in params.split(",")])
    return out


def structures():
    """{name: [(field, type text, array length | None)]} of every `typedef struct name { ... } name;`"""
    out = {}
    for name, body, alias in re.findall(r"typedef struct (\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", _header()):
        assert name == alias
        fields = []
        for decl in (d.strip() for d in body.split(";")):
            if not decl:
                continue
            first, *more = [x.strip() for x in decl.split(",")]            # `uint32_t a, b;` and `const char *a, *b;`
            m = re.match(r"^(.*?)(\**)\s*(\w+)(?:\[(\d+)\])?$", first)
            assert m and m.group(1).strip(), decl
            items = [m.groups()[1:]] + [re.match(r"^(\**)\s*(\w+)(?:\[(\d+)\])?$", x).groups() for x in more]
            for star, field, length in items:
                fields.append((field, m.group(1).strip() + (" *" if star else ""), int(length) if length else None))
        out[name] = fields
    return out


PROTOS = prototypes()


def test_the_parser_reads_the_header():
    """known prototypes and fields, by hand: the comparison below rests on this parser"""
    assert PROTOS["lva_version"] == ("constchar*", [])
    assert PROTOS["lva_decoder_destroy"] == ("void", ["lva_decoder *"])
    assert PROTOS["lva_stream_submit"] == ("int", ["lva_stream *", "const float *", "int64_t", "int32_t", "uint64_t"])
    assert len(PROTOS["lva_demux_bases_batch"][1]) == 11 and len(PROTOS["lva_list_filter"][1]) == 13
    s = structures()
    assert s["lva_payload_pos"] == [(k, "int32_t", None) for k in ("start_pos", "end_pos", "dist_start", "dist_end", "rc", "ok")]
    assert s["lva_experiment_barcodes"] == [("start_barcode", "const char *", None), ("end_barcode", "const char *", None),
                                            ("min_len", "uint32_t", None)]
    assert ("fixup_reason", "uint64_t", 4) in s["lva_profile"] and ("pattern", "uint8_t", 16) in s["lva_code_info"]
    assert s["lva_demux_pos"][0] == ("pos", "lva_payload_pos", None)


def test_the_table_names_exactly_the_functions_of_the_header():
    assert set(PROTOS) == set(_lib.ABI) and len(PROTOS) >= 42
    assert _lib.EXPORTS == list(_lib.ABI)


@pytest.mark.parametrize("name", sorted(_lib.ABI))
def test_prototype(name):
    ret, params = PROTOS[name]
    restype, argtypes = _lib.ABI[name]
    assert ret in ("int", "constchar*", "void"), ret
    assert restype is {"int": ctypes.c_int, "constchar*": ctypes.c_char_p, "void": None}[ret]
    assert len(argtypes) == len(params), (len(argtypes), params)
    for k, (t, decl) in enumerate(zip(argtypes, params)):
        assert _ctype_class(t) == _c_class(decl), "argument %d: %s against %r" % (k, t.__name__, decl)


def test_the_loaded_library_carries_the_table():
    L = _lib.load_library()
    for name, (restype, argtypes) in _lib.ABI.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes or []) == list(argtypes), name


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_structure(name):
    fields = structures()[name]
    cls = STRUCTS[name]
    assert [f for f, _, _ in fields] == [f for f, _ in cls._fields_]
    for (field, decl, length), (_, t) in zip(fields, cls._fields_):
        if length is not None:
            assert issubclass(t, ctypes.Array) and t._length_ == length, field
            t = t._type_
        else:
            assert not issubclass(t, ctypes.Array), field
        if decl in STRUCTS:
            assert t is STRUCTS[decl], field
        else:
            assert _ctype_class(t) == _c_class(decl), "%s: %s against %r" % (field, t.__name__, decl)


def test_every_structure_of_the_header_is_compared():
    assert set(structures()) == set(STRUCTS)
