"""The C ABI as Python reads it: prototypes and integer constants parsed from include/text_alignment_amd.h.

The header is the one place a signature or a constant is written down; hipcc holds the definitions in csrc/ against
it, and this module holds every ctypes binding (the package's and the tests') against it.  It imports neither torch
nor the library, so the host simulators of the tests can use it.

What the header may contain is deliberately little (the rule is stated at its top): plain C declarations
`RET NAME(PARAMS);` over stdint types, int, float, double, char, void and pointers to them, and object-like
`#define TA_NAME <integer expression>`.  Anything else is an error here, not a guess.
"""
import ctypes
import os
import re

HEADER = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include",
                                       "text_alignment_amd.h"))


class AbiError(RuntimeError):
    pass


_VALUES = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = set(_VALUES) | {"void", "char", "int8_t", "uint8_t", "int16_t", "uint16_t"}
_DECL = re.compile(r"^([\w\s\*]+?)\b(\w+)\s*\((.*)\)$", re.S)
_TOKEN = re.compile(r"\s*(?:(0[xX][0-9a-fA-F]+|0|[1-9]\d*)(?:[uU]?(?:LL|ll|L|l)?)(?!\w)|(\w+)|(<<|[()-]))")


def _ctype(text, what):
    """the ctypes type of one parameter or return type, `text` with or without the parameter's name"""
    words = re.findall(r"\w+|\*|\[\s*\d*\s*\]", text)
    if "".join(words) != re.sub(r"\s+", "", text):
        raise AbiError("cannot read %s: %r" % (what, text))
    words = [w for w in words if w != "const"]
    if not words:
        raise AbiError("cannot read %s: %r" % (what, text))
    base, rest = words[0], words[1:]
    levels = sum(1 for w in rest if w == "*" or w.startswith("["))
    names = [w for w in rest if w != "*" and not w.startswith("[")]
    if len(names) > 1 or base not in _POINTEES:
        raise AbiError("unknown type in %s: %r" % (what, text))
    if levels:
        return ctypes.c_char_p if (base == "char" and levels == 1) else ctypes.c_void_p
    if base not in _VALUES:
        raise AbiError("unknown type in %s: %r" % (what, text))
    return _VALUES[base]


def _constant(text, known, name):
    """the value of an integer expression: literals with u / L / LL suffixes, parentheses, unary minus, <<, names
    defined before it, INT64_MIN.  A recursive descent over exactly that grammar -- nothing is handed to eval."""
    toks, pos = [], 0
    while text[pos:].strip():
        m = _TOKEN.match(text, pos)
        if not m:
            raise AbiError("#define %s: cannot read the value %r" % (name, text))
        toks.append(m.groups())
        pos = m.end()
    toks.reverse()

    def primary():
        if not toks:
            raise AbiError("#define %s: the value %r ends early" % (name, text))
        lit, word, op = toks.pop()
        if lit is not None:
            return int(lit, 0)
        if word is not None:
            if word not in known:
                raise AbiError("#define %s: %r is not a constant defined before it" % (name, word))
            return known[word]
        if op == "-":
            return -primary()
        if op == "(":
            v = expr()
            if not toks or toks.pop()[2] != ")":
                raise AbiError("#define %s: unbalanced parentheses in %r" % (name, text))
            return v
        raise AbiError("#define %s: cannot read the value %r" % (name, text))

    def expr():
        v = primary()
        while toks and toks[-1][2] == "<<":
            toks.pop()
            v <<= primary()
        return v

    v = expr()
    if toks:
        raise AbiError("#define %s: cannot read the value %r" % (name, text))
    return v


def parse(text):
    """(prototypes, constants) of a header's text: name -> (restype, argtypes) in order of declaration, name -> int"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts, known, code = {}, {"INT64_MIN": -2 ** 63}, []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = re.match(r"\s*#\s*define\s+(TA_\w+)(\(?)(.*)$", line)
        if m and not m.group(2) and m.group(3).strip():          # object-like, with a value
            consts[m.group(1)] = known[m.group(1)] = _constant(m.group(3), known, m.group(1))
    code, wrapped = re.subn(r'extern\s+"C"\s*\{', " ", "\n".join(code))
    pieces = [p.strip() for p in code.split(";")]
    protos = {}
    for piece in pieces[:-1]:
        m = _DECL.match(piece)
        if not m:
            raise AbiError("not a declaration `RET NAME(PARAMS)`: %r" % piece)
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        if name in protos:
            raise AbiError("%s is declared twice" % name)
        args = [] if params == "void" else [_ctype(p, "a parameter of " + name) for p in params.split(",")]
        protos[name] = (_ctype(ret, "the return type of " + name), args)
    if pieces[-1] != ("}" if wrapped else ""):
        raise AbiError("text after the last declaration: %r" % pieces[-1])
    return protos, consts


def _read():
    try:
        with open(HEADER) as f:
            return f.read()
    except OSError as e:
        raise AbiError("the C header the binding is derived from is missing: %s (%s)" % (HEADER, e))


PROTOTYPES, CONSTANTS = parse(_read())


def bind(lib, names=None):
    """restype and argtypes of the header's symbols on a loaded library: all of them (names=None; one the library lacks
    is an error), or exactly those named"""
    for name in (PROTOTYPES if names is None else names):
        if name not in PROTOTYPES:
            raise AbiError("%s is not declared in %s" % (name, HEADER))
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise AbiError("%s is declared in %s but the library does not export it" % (name, HEADER))
        fn.restype, fn.argtypes = PROTOTYPES[name]
    return lib
