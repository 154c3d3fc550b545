"""Every compile-time switch the HIP sources test is listed in DESIGN.md's "Compile-time
switches" table, so that an undocumented experiment arm cannot be left behind in csrc."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tested_macros():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "mamba.jl_amd", "csrc", "*")):
        for line in open(path, encoding="utf-8"):
            m = re.match(r"\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)", line)
            if m:
                cond = m.group(1).split("//")[0]
                names.update(n for n in re.findall(r"[A-Za-z_]\w*", cond) if n != "defined")
    # the compiler's own names and include guards (NAME_H) are not switches
    return {n for n in names if not n.startswith("__") and not n.endswith("_H")}


def test_every_tested_macro_is_in_the_design_table():
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    section = design.split("### 4.7 Compile-time switches", 1)[1].split("\n## ", 1)[0]
    listed = set(re.findall(r"^\| `(\w+)` \|", section, flags=re.M))
    tested = _tested_macros()
    assert len(tested) >= 20, tested   # the scan found the sources
    assert tested <= listed, f"not in DESIGN.md's switch table: {sorted(tested - listed)}"
