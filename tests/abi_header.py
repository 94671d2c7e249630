"""include/hank_hip.h as data: every prototype's return class and parameter classes, and hank_model's fields. A parameter is a
pointer ("ptr": `T *x`, `T x[n]`), an "i32" (int32_t) or an "f64" (double); a function returns "int" or a "str" (const char *)."""
import re
from collections import namedtuple
from pathlib import Path

HEADER = Path(__file__).resolve().parent.parent / "include" / "hank_hip.h"
Proto = namedtuple("Proto", "ret params")


def _source():
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _param_class(decl):
    if "*" in decl or "[" in decl:
        return "ptr"
    for word, cls in (("int32_t", "i32"), ("double", "f64")):
        if re.search(r"\b" + word + r"\b", decl):
            return cls
    raise ValueError(f"a parameter of no known class: {decl!r}")


def prototypes():
    """{symbol: Proto(ret, (class of every parameter, ...))} in the header's order"""
    out = {}
    for ret, name, params in re.findall(r"\b(int|const\s+char\s*\*)\s*(hank_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", _source()):
        params = " ".join(params.split())
        out[name] = Proto("int" if ret == "int" else "str", () if params == "void" else tuple(_param_class(p) for p in params.split(",")))
    return out


def model_fields():
    """[(field, class)] of the struct hank_model; a pointer to doubles is "ptr_f64" """
    body = re.search(r"typedef\s+struct\s*\{(.*?)\}\s*hank_model\s*;", _source(), flags=re.S).group(1)
    fields = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        cls = "ptr_f64" if re.search(r"\bdouble\s*\*", decl) else _param_class(decl)
        names = re.sub(r"^(const\s+)?(int32_t|double)\s*\*?", "", decl)
        fields += [(n.strip(" *"), cls) for n in names.split(",")]
    return fields
