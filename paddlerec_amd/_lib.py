"""ctypes binding of librecengine.so — the only door from Python into the HIP kernels.

include/recengine.h is the single source: its constants, structs and prototypes are parsed at import
(parse_header) and nothing of it is repeated here.  A new entry point reaches Python by being declared in the
header; a new struct additionally gets its Python name in _STRUCT_NAMES.

There is no CPU fallback: if the library is missing or a call fails, an exception is raised.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librecengine.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "recengine.h")


class RecError(RuntimeError):
    pass


_SCALARS = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
            "float": C.c_float, "size_t": C.c_size_t, "int": C.c_int}
_POINTEES = ("void", "char", "uint8_t")          # known types that appear behind a '*' only
_DIRECTIVE = re.compile(r"#\s*(?:ifn?def\s+\w+|endif|include\s*<\w+\.h>|define\s+RECENGINE_H_)")
_DEFINE = re.compile(r"#\s*define\s+(REC_\w+)\s+(\S.*)")
_DECL = re.compile(r"\s*(?:(typedef\s+)?(enum|struct)\s*\{([^{}]*)\}\s*(\w*)\s*;|([^;{}]+);)")
_PROTO = re.compile(r"(const\s+)?(\w+)\s*(\*?)\s*(rec_\w+)\s*\((.*)\)", re.S)
_PARAM = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)")
_FIELD = re.compile(r"(?:const\s+)?(\w+)\b(.*)", re.S)
_DECLARATOR = re.compile(r"(\*?)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?")


def _int(expr, consts, decl):
    """Value of an integer constant expression over literals, ( ), <<, + - * | and earlier constants."""
    try:
        if not re.fullmatch(r"(?:<<|[-\w+*|()\s])+", expr):
            raise ValueError(expr)
        value = eval(expr, {"__builtins__": {}}, consts)  # only names of `consts` and the operators above get here
    except Exception:
        raise RecError("recengine.h: cannot evaluate %r in %r" % (expr, decl)) from None
    if type(value) is not int:
        raise RecError("recengine.h: %r in %r is not an integer" % (expr, decl))
    return value


def parse_header(text, struct_names=None):
    """Header text -> (constants {REC_X: int}, structs {rec_name: ctypes.Structure class}, signatures
    {rec_name: (restype, argtypes)}).  struct_names maps a struct's C name to the name of its Python class.  Anything
    that is not recognised raises RecError naming the declaration; nothing is skipped."""
    struct_names = struct_names or {}
    consts, structs, sigs, body = {}, {}, {}, []
    for line in re.sub(r"/\*.*?\*/", " ", text, flags=re.S).splitlines():
        if not line.lstrip().startswith("#"):
            body.append(line)
            continue
        m = _DEFINE.fullmatch(line.strip())
        if m:
            consts[m.group(1)] = _int(m.group(2), consts, line.strip())
        elif not _DIRECTIVE.fullmatch(line.strip()):
            raise RecError("recengine.h: unrecognised directive %r" % line.strip())
    body = "\n".join(body)
    m = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', body, re.S)
    body = m.group(1) if m else body

    def pointee(name, decl):
        if name not in _SCALARS and name not in _POINTEES and name not in structs:
            raise RecError("recengine.h: unknown type %r in %r" % (name, decl))
        return C.c_void_p

    def by_value(name, decl):
        if name not in _SCALARS and name not in structs:
            raise RecError("recengine.h: unknown type %r in %r" % (name, decl))
        return _SCALARS.get(name) or structs[name]

    def fields_of(members, decl):
        fields = []
        for member in filter(None, (s.strip() for s in members.split(";"))):
            m = _FIELD.fullmatch(member)
            for declarator in (m.group(2).split(",") if m else [""]):
                d = _DECLARATOR.fullmatch(declarator.strip())
                if not d:
                    raise RecError("recengine.h: unrecognised field %r in %s" % (member, decl))
                star, name, extent = d.groups()
                ctype = pointee(m.group(1), member) if star else by_value(m.group(1), member)
                fields.append((name, ctype * _int(extent, consts, member) if extent else ctype))
        return fields

    def prototype(decl):
        m = _PROTO.fullmatch(decl)
        if not m or m.group(4) in sigs:
            raise RecError("recengine.h: cannot place declaration %r" % decl)
        const, ret, star, name, params = m.groups()
        if star and not (const and ret == "char"):
            raise RecError("recengine.h: unsupported return type in %r" % decl)
        argtypes = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            p = _PARAM.fullmatch(param.strip())
            if not p:
                raise RecError("recengine.h: unrecognised parameter %r of %s" % (param.strip(), name))
            base, stars = p.group(1), p.group(2).count("*")
            if stars == 1 and base in structs:
                argtypes.append(C.POINTER(structs[base]))
            else:
                argtypes.append(pointee(base, decl) if stars else by_value(base, decl))
        sigs[name] = (C.c_char_p if star else by_value(ret, decl), argtypes)

    pos = 0
    while body[pos:].strip():
        m = _DECL.match(body, pos)
        if not m:
            raise RecError("recengine.h: cannot place declaration %r" % body[pos:].strip()[:80])
        pos = m.end()
        typedef, kind, members, name, other = m.groups()
        if kind == "enum":
            for item in filter(None, (s.strip() for s in members.split(","))):
                e = re.fullmatch(r"(REC_\w+)\s*=\s*(.+)", item, re.S)
                if not e:
                    raise RecError("recengine.h: enumerator %r has no explicit value" % item)
                consts[e.group(1)] = _int(e.group(2), consts, item)
        elif kind == "struct":
            if not typedef or not name or name in structs:
                raise RecError("recengine.h: cannot place declaration 'struct { ... } %s'" % name)
            structs[name] = type(struct_names.get(name, name), (C.Structure,),
                                 {"_fields_": fields_of(members, name), "__doc__": name + " (include/recengine.h)."})
        else:
            prototype(" ".join(other.split()))
    return consts, structs, sigs


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise RecError("cannot read the engine's header %s: %s" % (HEADER_PATH, e)) from None


# Python class <- struct of the header
_STRUCT_NAMES = dict(
    rec_deepfm_desc="DeepFMDesc", rec_ffm_desc="FFMDesc", rec_fatffm_desc="FatFFMDesc", rec_fefm_desc="FEFMDesc",
    rec_dcn_cross_desc="DcnCrossDesc", rec_deepfm_net="DeepFMNet", rec_din_net="DinNet", rec_dcn_v2_net="DcnV2Net",
    rec_adam_hyper="AdamHyper", rec_adagrad_hyper="AdagradHyper", rec_grad_layout="GradLayout",
    rec_small_sgd_job="SmallSgdJob", rec_cin_view="CinView", rec_ps_accessor="PsAccessor", rec_lazy_init="LazyInit",
    rec_ps_layout="PsLayout", rec_grad_src="GradSrc", rec_multislot_desc="MultislotDesc", rec_din_desc="DinDesc",
    rec_crossnet_v2_desc="CrossV2Desc", rec_crossnet_mix_desc="CrossMixDesc", rec_gemm_desc="GemmDesc",
    rec_gemm_epilogue_args="GemmEpilogueArgs", rec_gemm_route="GemmRoute", rec_mtl_mix_desc="MtlMixDesc",
    rec_esm_head_desc="EsmHeadDesc", rec_aitm_head_desc="AitmHeadDesc", rec_ids_group_plan_t="IdsGroupPlan",
    rec_gemm_b_image="GemmBImage")

# CONSTANTS: every REC_* macro and enumerator; STRUCTS: by C name; SIGNATURES: name -> (restype, argtypes)
CONSTANTS, STRUCTS, SIGNATURES = parse_header(_read_header(), _STRUCT_NAMES)
globals().update(CONSTANTS)
globals().update((_STRUCT_NAMES[c_name], cls) for c_name, cls in STRUCTS.items() if c_name in _STRUCT_NAMES)

STRUCTS["rec_deepfm_net"].MAX_LINEAR = CONSTANTS["REC_DEEPFM_MAX_LINEAR"]
DCN_MAX_LAYERS = CONSTANTS["REC_DCN_MAX_LAYERS"]
EPI = {name[len("REC_EPI_"):].lower(): value for name, value in CONSTANTS.items() if name.startswith("REC_EPI_")}
GEMM_ROUTE_FAMILIES = ("skinny_rows", "skinny_dw", "x3_dw", "x3", "panel", "glds", "direct", "tiled")
GEMM_ROUTE_FLAGS = dict(fast=1, pipe=2, vec=4, ks4=8, fold=16, vec_a=32, pair=64)
GEMM_CFGS = ("128x80", "256x80", "256x128", "128x128", "80x80", "64x80", "128x80_o4", "144x80")  # gemm_f32.hip's

_lib = None


def lib():
    """Load librecengine.so (once).  Raises RecError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RecError(
                "librecengine.so not found at %s — run `python -m paddlerec_amd.build` "
                "(there is no CPU fallback)" % LIB_PATH)
        # PyTorch-ROCm wheels bundle their own libamdhip64; it must be the HIP runtime of the process.  If
        # librecengine.so were loaded first it would pull in /opt/rocm's copy and the process would end up
        # with two runtimes ("no ROCm-capable device is detected" on the first launch) — so torch goes first.
        import torch  # noqa: F401
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(h, name)  # AttributeError if the symbol is missing
            fn.restype, fn.argtypes = res, args
        _lib = h
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().rec_last_error().decode("utf-8", "replace")
        raise RecError("%s failed (rc=%d): %s" % (what or "recengine call", rc, msg))
