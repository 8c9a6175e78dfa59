"""The interfaces between the translation units of csrc/ are written once (DESIGN.md "File layout"): a function that
crosses a file is declared in a header that its defining file includes too, and a type that crosses a file is defined in
a header.  Two properties of the source text keep it so — no compiler, no library, no device:
  (a) no struct / class / enum name with a body is defined in more than one file;
  (b) no .hip / .cpp file declares a function at column 0 without defining it (a prototype copied from another file:
      a parameter list that drifts is a link error at best, a return type or default argument that drifts is nothing)."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ptbxl-multimodal_amd", "csrc")

TYPE_BODY = re.compile(r"\b(?:struct|class|enum(?:\s+(?:class|struct))?)\s+(\w+)\s*(?::[^;{()]*)?\{")
# `static`, `extern`, `template`, `typedef` and `using` lines are something else; `return f(x);` is no declaration
PROTOTYPE = re.compile(r"^(?!static\b|return\b|typedef\b|using\b|template\b|extern\b)(?:[\w:<>]+[\s\*&]+)+(\w+)\(([^(){};]*)\)\s*;",
                       re.M)


def _sources():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".cpp", ".h")):
            with open(os.path.join(CSRC, name)) as f:
                text = f.read()
            text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
            out[name] = re.sub(r"//[^\n]*", "", text)          # comments may quote either form; line numbers are kept
    assert len(out) >= 20, "csrc/ not found where the test looks for it: %s" % CSRC
    return out


def test_no_type_is_defined_in_two_files():
    where = {}
    for name, text in _sources().items():
        for t in set(TYPE_BODY.findall(text)):
            where.setdefault(t, []).append(name)
    twice = {t: files for t, files in where.items() if len(files) > 1}
    assert not twice, "defined in more than one file of csrc/ (move it to a header): %s" % twice


def test_no_source_file_declares_a_function_it_does_not_define():
    found = []
    for name, text in _sources().items():
        if name.endswith(".h"):
            continue
        for m in PROTOTYPE.finditer(text):
            found.append("%s:%d %s" % (name, text.count("\n", 0, m.start()) + 1, m.group(1)))
    assert not found, "prototypes in source files of csrc/ (declare them in a header the defining file includes): %s" % found


def test_the_patterns_see_what_they_are_for():
    """the two expressions on text of the forms they exist to find, and on what they must leave alone"""
    assert TYPE_BODY.findall("struct RingPlan { bool ok; };\nenum Epilogue { A = 0 };\nenum class E : int { B };") == \
        ["RingPlan", "Epilogue", "E"]
    assert TYPE_BODY.findall("struct RingPlan;\nenum { WGR = 0 };\nconst RingPlan rp{true, 1};\nvoid f(struct stat *s) {") == []
    hit = ("int wgrad_reduce(const float *ws, float *dw, size_t wslab, hipStream_t st);\n"
           "RingPlan bf16_ring_plan(int N, int Cin,\n                        bool xf32 = false);\n"
           "const float *row_of(int n);\n")
    assert [m.group(1) for m in PROTOTYPE.finditer(hit)] == ["wgrad_reduce", "bf16_ring_plan", "row_of"]
    miss = ("static int f(int a);\nextern \"C\" int g(int a);\nint h(int a) { return a; }\n    int inner(int a);\n"
            "return fail(1, 2);\ntemplate <int N> void k(int a);\nusing F = int (*)(int);\n")
    assert [m.group(1) for m in PROTOTYPE.finditer(miss)] == []
