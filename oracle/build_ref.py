"""Recipe run by build(): byte-compile the reference's `ppeadepth` package into oracle/_ref/ppeadepth/ as sourceless
.pyc files, so that CPU tests which exercise the unmodified reference code (tests/test_plugin.py) need only the working
tree.  Where the reference tree is not readable, an existing oracle/_ref is left as it is.  oracle/_ref is ignored by
git: nothing compiled from the reference is ever committed."""
import os
import py_compile
import shutil

from oracle.ref_harness import COMPILED_ROOT, REFERENCE_ROOT


def build():
    """-> True when oracle/_ref was (re)built from the reference tree."""
    src = os.path.join(REFERENCE_ROOT, "ppeadepth")
    if not os.access(src, os.R_OK | os.X_OK):
        return False
    dst = os.path.join(COMPILED_ROOT, "ppeadepth")
    tmp = dst + ".tmp"
    shutil.rmtree(tmp, ignore_errors=True)
    for d, _, files in os.walk(src):
        for f in files:
            if f.endswith(".py"):
                rel = os.path.relpath(os.path.join(d, f), src)
                py_compile.compile(os.path.join(d, f), cfile=os.path.join(tmp, rel[:-3] + ".pyc"),
                                   dfile=os.path.join("ppeadepth", rel), doraise=True)
    shutil.rmtree(dst, ignore_errors=True)
    os.replace(tmp, dst)
    return True
