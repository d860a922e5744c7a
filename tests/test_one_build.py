"""There is one build of the kernel sources: no preprocessor conditional selects a variant of them.

The only TE_ macro a conditional may test is TE_PATH_COUNTERS, the CPU harness's coverage counters.  Needs no build.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONDITIONAL = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")


def test_no_conditional_tests_a_te_macro():
    found, scanned = [], 0
    for path in sorted(glob.glob(os.path.join(ROOT, "drl-tetris_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "tests", "cpu_harness", "*"))):
        if not path.endswith((".h", ".hip", ".c", ".cpp")):
            continue
        scanned += 1
        with open(path, encoding="utf-8") as f:
            for n, line in enumerate(f, 1):
                m = CONDITIONAL.match(line)
                for macro in re.findall(r"\bTE_\w+", m.group(2)) if m else ():
                    if macro != "TE_PATH_COUNTERS":
                        found.append(f"{os.path.relpath(path, ROOT)}:{n}: {line.strip()}")
    assert scanned >= 10, "the kernel sources were not found"
    assert not found, "compile-time variants of the kernel sources:\n" + "\n".join(found)
