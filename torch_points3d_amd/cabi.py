"""ctypes signatures read from the C headers, so that include/tp3d_hip.h and include/tp3d_cpu.h are the only statement of
the ABI: the compiler checks every definition against them (TP3D_EXPORT), and the Python bindings are derived here.

Only the C subset those two headers use is understood; anything else raises ValueError naming the declaration, never a
guessed type."""
import ctypes
import re

_VALUE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double,
          "size_t": ctypes.c_size_t}
_NOT_A_NAME = set(_VALUE) | {"void", "char", "const", "volatile", "unsigned", "signed", "long", "short", "struct", "enum",
                                "union"}
_RETURN = dict(_VALUE, **{"void": None, "void *": ctypes.c_void_p, "const char *": ctypes.c_char_p})
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+|\(-?\d+\))[ \t]*$", re.M)
_DECL = re.compile(r"(.*?)\b(\w+) ?\(([^()]*)\)$")


def _tokens(text):
    return re.findall(r"\w+|\S", text)


def _is_name(word):
    return word.isidentifier() and word not in _NOT_A_NAME


def _argtype(param, decl):
    tok = _tokens(param)
    value = tok[1:] if tok[:1] == ["const"] else tok
    if len(value) == 2 and value[0] in _VALUE and _is_name(value[1]):
        return _VALUE[value[0]]
    # a pointer: type words and stars ("const float *const *xs", "unsigned char *arg"), then the name
    if "*" in tok[1:-1] and tok[0].isidentifier() and _is_name(tok[-1]) and all(
            t == "*" or t.isidentifier() for t in tok[:-1]):
        return ctypes.c_void_p
    raise ValueError("unsupported parameter %r in declaration %r" % (param.strip(), decl))


def parse(text):
    """(functions, constants) of a header's text: name -> (restype, [argtypes]) and NAME -> int of the integer #defines"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {name: int(value.strip("()")) for name, value in _DEFINE.findall(text)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    *statements, tail = text.split(";")
    if tail.strip() not in ("", "}"):
        raise ValueError("declaration without ';': %r" % " ".join(tail.split()))
    functions = {}
    for decl in statements:
        decl = " ".join(decl.split())
        m = _DECL.match(decl)
        restype = " ".join(_tokens(m.group(1))) if m else None
        if restype not in _RETURN:
            raise ValueError("not a function declaration of the supported subset: %r" % decl)
        params = [] if m.group(3).strip() == "void" else m.group(3).split(",")
        functions[m.group(2)] = (_RETURN[restype], [_argtype(p, decl) for p in params])
    return functions, constants


def parse_header(path):
    with open(path) as f:
        return parse(f.read())
