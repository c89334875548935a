"""include/mvs_hip.h read as the one statement of the C ABI: ctypes prototypes, status-returning functions, numeric constants.

The header is plain C with a closed vocabulary (below); anything outside it raises - a prototype is never guessed."""
import ctypes as C
import os
import re

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mvs_hip.h")
SCALARS = {"int": C.c_int, "mvs_status": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           "long long": C.c_longlong, "unsigned long long": C.c_ulonglong}


def _ctype(decl: str, where: str, result: bool = False):
    """One parameter (its name is optional) or one return type -> ctypes type."""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        if result and words != ["const", "char", "*"]:
            raise ValueError("mvs_hip.h: %s: return type '%s' is outside the binding's vocabulary" % (where, decl))
        return C.c_char_p if result else C.c_void_p
    for n in (len(words), len(words) - 1 + result):           # the whole text is the type, or its last word is the parameter's name
        if " ".join(words[:n]) in SCALARS:
            return SCALARS[" ".join(words[:n])]
    raise ValueError("mvs_hip.h: %s: type '%s' is outside the binding's vocabulary" % (where, decl))


def parse(text: str):
    """-> (prototypes {name: (restype, argtypes)}, names of the functions declared mvs_status, constants {MVS_X: int})."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    consts = {k: int(v) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(MVS_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).replace('extern "C" {', "")
    protos, status = {}, set()
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if stmt.startswith("enum"):
            consts.update((k, int(v)) for k, v in re.findall(r"(MVS_\w+) = (-?\d+)", stmt))
        if not stmt or stmt == "}" or stmt.startswith(("enum", "typedef")):
            continue
        m = re.fullmatch(r"(.+?)\b(\w+) ?\((.*)\)", stmt)
        if m is None or m.group(2) in protos:
            raise ValueError("mvs_hip.h: cannot read the declaration '%s'" % stmt)
        res, name, params = m.groups()
        args = [] if params.strip() == "void" else [_ctype(p, name) for p in params.split(",")]
        protos[name] = (_ctype(res, name, result=True), args)
        if res.strip() == "mvs_status":
            status.add(name)
    return protos, frozenset(status), consts


PROTOTYPES, STATUS, CONSTANTS = parse(open(PATH).read())
