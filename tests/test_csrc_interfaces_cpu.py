"""The library's internal interfaces live in headers, one per producing source.

Every `.hip`, `.cpp` and `.hpp` under csrc/ is read with comments, string literals and preprocessor lines stripped
and split into its statements at namespace scope (`namespace x {` and `extern "C" {` are looked through; every other
brace pair is a body and is skipped).  A statement that ends in a body and names a function defines it; one that ends
in `;` and names a function declares it.  Two properties are asserted:

  * no function defined in one `.hip` / `.cpp` has a prototype in another `.hip` / `.cpp`: a hand-copied prototype
    is checked by name mangling for its parameter types only, not for a default argument, a return type or a meaning;
  * every header that declares such a function is included, directly or through other csrc headers, by the source
    that defines it, so the compiler compares the declaration with the definition.

Before the interface headers existed this parse found 33 such prototypes, counted per (source, function): 25 in
kl_closed.hip, 3 in predict.hip, 2 in potrf.hip, 2 in gram.hip and 1 in kl_cond.hip.  (The issue that asked for this
test named 27 for kl_closed.hip beside the same total of 33, but its per-source figures add to 35.  kl_closed.hip held
26 declarations, one of them `struct HbDev;`: 25 prototypes, and 33 in all is the count that holds.)
"""
import functools
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "longitudinal-vae_amd", "csrc")

_STRIP = re.compile(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'', re.S)
_ATTR = re.compile(r"\b(?:__launch_bounds__|__attribute__|alignas|decltype|noexcept)\s*\(")
_NAME = re.compile(r"([A-Za-z_]\w*)\s*\($")
_NOT_FUNCTIONS = {"static_assert", "if", "for", "while", "switch", "return", "sizeof", "operator"}


def _clean(text):
    """comments and literals out (`extern "C"` kept as the word extern_C), then preprocessor lines with their
    continuations"""
    text = text.replace('extern "C"', "extern_C")
    text = _STRIP.sub(" ", text)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", "", text, flags=re.M)
    return text


def _includes(path):
    with open(path) as f:
        return set(re.findall(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', _STRIP.sub(
            lambda m: m.group(0) if m.group(0).startswith('"') else " ", f.read()), flags=re.M))


def _drop_parens(stmt, start):
    """stmt with the balanced parenthesis group that opens at stmt[start] removed"""
    depth = 0
    for i in range(start, len(stmt)):
        depth += (stmt[i] == "(") - (stmt[i] == ")")
        if depth == 0:
            return stmt[:start] + " " + stmt[i + 1:]
    return stmt[:start]


def _function_name(stmt):
    """the name a namespace-scope statement declares or defines as a function, or None"""
    stmt = " ".join(stmt.split())
    if not stmt or stmt.split()[0] in ("typedef", "using", "struct", "class", "enum", "union"):
        return None
    while True:
        m = _ATTR.search(stmt)
        if not m:
            break
        stmt = _drop_parens(stmt[:m.start()] + stmt[m.end() - 1:], m.start())
    depth = 0  # (template argument lists may hold parentheses of their own: only depth-0 `(` counts)
    for i, ch in enumerate(stmt):
        if ch == "(":
            if depth == 0:
                if "=" in stmt[:i]:
                    return None  # an initialiser, not a declarator
                m = _NAME.search(stmt[:i + 1])
                return m.group(1) if m and m.group(1) not in _NOT_FUNCTIONS else None
            depth += 1
        elif ch == ")":
            depth -= 1
    return None


def parse(path):
    """(defined, declared): {name: is_static} of the functions the file defines at namespace scope, and the set of
    names it declares without a body"""
    with open(path) as f:
        text = _clean(f.read())
    defined, declared = {}, set()
    stmt, i, n = [], 0, len(text)
    while i < n:
        ch = text[i]
        if ch == ";":
            name = _function_name("".join(stmt))
            if name:
                declared.add(name)
            stmt = []
        elif ch == "{":
            head = " ".join("".join(stmt).split())
            if re.fullmatch(r"(?:inline )?namespace(?: \w+)?|extern_C", head):
                stmt = []  # looked through: its closing brace is dropped below
            else:
                depth = 1
                while depth:
                    i += 1
                    depth += (text[i] == "{") - (text[i] == "}")
                name = _function_name(head)
                if name:
                    defined[name] = bool(re.search(r"\bstatic\b", head)) or defined.get(name, False)
                    stmt = []
                elif "=" in head:
                    stmt.append(" ")  # a braced initialiser: the statement runs on to its `;`
                else:
                    stmt = []  # a struct, class or enum body; a trailing `;` is then an empty statement
        elif ch == "}":
            stmt = []
        else:
            stmt.append(ch)
        i += 1
    return defined, declared


@functools.lru_cache(maxsize=None)
def _tree(csrc):
    srcs = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.cpp")))
    hdrs = sorted(glob.glob(os.path.join(csrc, "*.hpp")))
    parsed = {os.path.basename(p): parse(p) for p in srcs + hdrs}
    incl = {os.path.basename(p): _includes(p) for p in srcs + hdrs}
    owner = {}  # external function -> the source that defines it
    for p in srcs:
        for name, static in parsed[os.path.basename(p)][0].items():
            if not static:
                owner.setdefault(name, os.path.basename(p))
    return [os.path.basename(p) for p in srcs], [os.path.basename(p) for p in hdrs], parsed, incl, owner


def copied_prototypes(csrc=CSRC):
    """[(source, function, defining source)]: prototypes in a .hip / .cpp of functions another one defines"""
    srcs, _, parsed, _, owner = _tree(csrc)
    return [(s, name, owner[name]) for s in srcs for name in sorted(parsed[s][1])
            if name in owner and owner[name] != s and name not in parsed[s][0]]


def _reach(src, incl):
    seen, todo = set(), [src]
    while todo:
        for h in incl.get(todo.pop(), ()):
            if h not in seen:
                seen.add(h)
                todo.append(h)
    return seen


def unchecked_headers(csrc=CSRC):
    """[(header, function, defining source)]: declarations the defining source never sees"""
    _, hdrs, parsed, incl, owner = _tree(csrc)
    return [(h, name, owner[name]) for h in hdrs for name in sorted(parsed[h][1])
            if name in owner and name not in parsed[h][0] and h not in _reach(owner[name], incl)]


def test_parser_sees_the_sources():
    """the parse is not vacuous: it finds the Gram sources' host functions and the headers' declarations"""
    srcs, hdrs, parsed, _, owner = _tree(CSRC)
    assert len(srcs) >= 20 and len(hdrs) >= 20
    for name, src in [("kl_gram_fill", "kl_gram.hip"), ("kl_gram_bwd", "kl_gram.hip"),
                      ("gram_matvec_f64", "gram_matvec.hip"), ("kl_gram_resid", "gram_matvec.hip"),
                      ("gram_multi_f64", "gram.hip"), ("lvae_gram_f64", "gram.hip"),
                      ("ci_factor_f32", "chol_inv.hip"), ("syrk_tiles_f32", "syrk_x3.hip"),
                      ("kl_hyper_bwd", "kl_hyper.hip"), ("kl_resid_bins", "kl_resid_bins.hip"),
                      ("kl_refine_gate", "kl_refine.hip")]:
        assert owner.get(name) == src, (name, owner.get(name))
    for name, hdr in [("kl_gram_fill", "gram.hpp"), ("gram_matvec_comp_f64", "gram.hpp"),
                      ("ci_factor_f32", "chol_inv.hpp"), ("syrk_x3_splits", "syrk_x3.hpp"),
                      ("kl_hyper_plan", "kl_hyper.hpp"), ("kl_resid_bins_plan", "kl_resid_bins.hpp"),
                      ("kl_refine_diag", "kl_refine.hpp")]:
        assert name in parsed[hdr][1], (name, hdr)
    # statics, kernels and device helpers are definitions too, and never taken for prototypes
    assert parsed["gram_tile.hpp"][0].get("spec_qs") is True and parsed["gram_tile.hpp"][0].get("tri_index") is False
    assert "gram_kernel" in parsed["gram.hip"][0] and "gram_kernel" not in parsed["gram.hip"][1]


def test_parser_finds_a_copied_prototype_and_an_unchecked_header(tmp_path):
    """both checks fire on a three-file tree that breaks them, and only on what breaks them"""
    (tmp_path / "a.hip").write_text('#include "b.hpp"\nnamespace lvae {\n'
                                    "int f(int x, float* y = nullptr);  // a copy, with a default of its own\n"
                                    "static int helper(int);\nstatic int helper(int x) { return x; }\n"
                                    "int g(int x) { return f(helper(x)); }\n}\n")
    (tmp_path / "b.hip").write_text("namespace lvae {\n/* int g(int); */\nint f(int x, float* y) { return x; }\n"
                                    'const char* s = "int g(int);";\n}\nextern "C" {\nint c_entry(void) { return 0; }\n}\n')
    (tmp_path / "b.hpp").write_text("#pragma once\nnamespace lvae {\nint f(int x, float* y);\nint g(int x);\n"
                                    "inline int h(int x) { return x; }\n}\n")
    assert copied_prototypes(str(tmp_path)) == [("a.hip", "f", "b.hip")]
    assert unchecked_headers(str(tmp_path)) == [("b.hpp", "f", "b.hip")]


def test_no_prototype_of_another_sources_function():
    assert copied_prototypes() == []


def test_every_interface_header_is_included_by_its_source():
    assert unchecked_headers() == []
