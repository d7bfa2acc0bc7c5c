"""CPU check of how the HIP back-end (bcnn_amd/csrc) declares what crosses its source files. A function of the library
that one .hip file defines and another one calls has ONE prototype, in a header, and its default arguments live there:
a hand-copied prototype in the calling file keeps compiling and linking when a default argument changes or a parameter
of the same type is inserted, and then calls the function wrongly. The weight-gradient kernels' common "workspace too
small" exit has one copy too (conv_common.h: conv_require_workspace)."""
import glob
import os
import re

from tests.test_scratch_ownership import CSRC, _strip_comments

_NOT_A_NAME = {"__launch_bounds__", "__attribute__", "alignas", "__declspec", "static_assert"}
_SCOPE = re.compile(r'^(?:inline\s+)?namespace\b[^(]*$|^extern\s+"C"$')
_DEVICE_CODE = re.compile(r"\b__global__\b|\b__device__\b")


def _blank(text):
    """preprocessor lines and the contents of string / character literals blanked out, so that braces, parentheses and
    semicolons that are left are the language's own"""
    text = re.sub(r"^[ \t]*#(?:[^\n\\]|\\\n|\\.)*", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.M)
    return re.sub(r'"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'',
                  lambda m: m.group(0) if m.group(0) == '"C"' else m.group(0)[0] * 2, text)


def _functions(text):
    """(name, 'decl' | 'def', is_static, in_extern_c, is_device_code, parameter text) of every function declared or
    defined at namespace scope in comment-stripped source"""
    text = _blank(text)
    out, scopes, i, start, n = [], [], 0, 0, len(text)
    while i < n:
        ch = text[i]
        if ch == "(":  # to the matching parenthesis: default arguments and attributes may hold anything
            depth = 1
            while depth:
                i += 1
                depth += {"(": 1, ")": -1}.get(text[i], 0)
        elif ch == "}":  # only a scope can close here: every other brace pair is skipped as a whole below
            scopes.pop()
            start = i + 1
        elif ch in ";{":
            head = " ".join(text[start:i].split())
            if ch == "{" and _SCOPE.match(head):
                scopes.append("C" if head.startswith("extern") else "ns")
            else:
                if ch == "{":
                    depth = 1
                    while depth:
                        i += 1
                        depth += {"{": 1, "}": -1}.get(text[i], 0)
                head = re.sub(r"^(?:template\s*<[^{};]*?>\s*)+", "", head)
                paren = head.find("(")
                if paren > 0 and "=" not in head[:paren] and not re.match(r"(?:typedef|using|struct|class|enum)\b", head):
                    names = [m for m in re.finditer(r"\b(\w+)\s*\(", head) if m.group(1) not in _NOT_A_NAME and
                             head.count("(", 0, m.start()) == head.count(")", 0, m.start())]
                    if names and not head[:names[0].start()].rstrip("~").endswith("::"):  # (a member function is its class's)
                        m, depth, j = names[0], 1, names[0].end()
                        while depth:
                            depth += {"(": 1, ")": -1}.get(head[j], 0)
                            j += 1
                        out.append((m.group(1), "decl" if ch == ";" else "def",
                                    bool(re.search(r"\bstatic\b", head[:m.start()])), "C" in scopes,
                                    bool(_DEVICE_CODE.search(head[:m.start()])), head[m.end():j - 1]))
            start = i + 1
        i += 1
    assert not scopes
    return out


def _parsed(pattern):
    paths = sorted(glob.glob(os.path.join(CSRC, pattern)))
    assert len(paths) > 10, paths
    texts = {os.path.basename(p): _strip_comments(open(p).read()) for p in paths}
    return texts, {fn: _functions(t) for fn, t in texts.items()}


def _cross_file_functions(texts, funcs):
    """name -> defining .hip file, for the library's own (not extern "C") host functions that another .hip file uses"""
    cross = {}
    for fn, fs in funcs.items():
        for name, kind, static, in_c, device, _ in fs:
            if kind != "def" or static or in_c or device:
                continue
            for other, text in texts.items():
                if other != fn and not any(f[0] == name for f in funcs[other] if f[1] == "def") and \
                        re.search(r"\b%s\b" % re.escape(name), text):
                    cross[name] = fn
    assert len(cross) > 40, sorted(cross)
    return cross


def test_no_hip_file_declares_a_function_it_does_not_define():
    _, funcs = _parsed("*.hip")
    for fn, fs in funcs.items():
        for name, kind, static, _, device, _ in fs:
            assert kind == "def" or static or device, \
                "%s: prototype of %s(); what crosses files is declared in a header, once" % (fn, name)


def test_cross_file_functions_are_declared_in_exactly_one_header():
    texts, funcs = _parsed("*.hip")
    _, hdr = _parsed("*.h")
    for name, fn in sorted(_cross_file_functions(texts, funcs).items()):
        where = [h for h, fs in hdr.items() for f in fs if f[0] == name and f[1] == "decl"]
        assert len(where) == 1, "%s() of %s is used by other files and declared in %s" % (name, fn, where or "no header")


def test_default_arguments_live_on_the_header_declaration():
    texts, funcs = _parsed("*.hip")
    cross = _cross_file_functions(texts, funcs)
    for fn, fs in funcs.items():
        for name, _, _, _, _, params in fs:
            assert name not in cross or "=" not in params, "%s: default argument of %s() outside its header" % (fn, name)


def test_the_workspace_check_has_one_copy():
    n = 0
    for p in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        n += open(p).read().count("workspace too small")
    assert n == 1


def _identifiers(fn):
    return set(re.findall(r"[A-Za-z_]\w*", _blank(_strip_comments(open(os.path.join(CSRC, fn)).read()))))


def test_the_fused_depthwise_families_do_not_know_each_other():
    """depthwise.hip's two tables order the families; of the other family's file only dwl_finalize_launch is called"""
    lds, march = _identifiers("depthwise_lds.hip"), _identifiers("depthwise_march.hip")
    assert not [i for i in lds if re.search(r"march", i, re.I)]
    assert not [i for i in march if re.search(r"depthwise_\w*lds", i)]
    defined = {f[0] for f in _functions(_strip_comments(open(os.path.join(CSRC, "depthwise_lds.hip")).read()))
               if f[1] == "def" and not f[2] and not f[4]}
    assert "dwl_finalize_launch" in defined and defined & march == {"dwl_finalize_launch"}


def test_the_depthwise_shape_is_derived_once():
    """the output-extent formula of a DwShape, and who may ask the marching family for its slots"""
    n, splits = 0, set()
    for p in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        text = _strip_comments(open(p).read())
        n += len(re.findall(r"DwShape\s*\w*\s*\{[^{};]*/\s*\w+\s*\+\s*1", text))
        if re.search(r"\bdepthwise_march_splits\b", text):
            splits.add(os.path.basename(p))
    assert n == 1
    assert splits == {"depthwise_march.hip", "depthwise.h", "depthwise.hip"}
    table = _strip_comments(open(os.path.join(CSRC, "depthwise.hip")).read())
    rows = re.findall(r"kDw(?:Fwd|Bwd)Families\[\]\s*=\s*\{(.*?)\n\};", table, re.S)
    assert len(rows) == 2 and table.count("depthwise_march_splits") == sum(r.count("depthwise_march_splits") for r in rows) == 2


def _parameter_count(params):
    """top-level commas of a parameter list + 1; brackets of any kind (templates, function pointers, array bounds) nest"""
    if params.strip() in ("", "void"):
        return 0
    depth = n = 0
    for ch in params:
        depth += {"(": 1, "[": 1, "{": 1, "<": 1, ")": -1, "]": -1, "}": -1, ">": -1}.get(ch, 0)
        n += ch == "," and depth == 0
    assert depth == 0, params
    return n + 1


def test_host_functions_behind_the_abi_take_at_most_13_parameters():
    """what the C ABI spreads over dozens of positional arguments travels in named structs behind it (batchnorm.h: BnFwdCall,
    BnBwdCall; conv.hip: ConvNodeFwd, ConvNodeBwd). 13 is lrn_run's count (lrn_dropout.hip), the largest there is."""
    assert _parameter_count("const ConvFamily<A, B> (&rows)[R], int (*f)(int, int), float x = g(1, 2)") == 3
    seen = 0
    for pattern in ("*.hip", "*.h"):
        for fn, fs in _parsed(pattern)[1].items():
            for name, _, _, in_c, device, params in fs:
                if in_c or device:
                    continue
                seen += 1
                assert _parameter_count(params) <= 13, "%s: %s() takes %d parameters" % (fn, name, _parameter_count(params))
    assert seen > 300, seen
