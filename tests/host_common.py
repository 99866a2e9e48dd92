"""What the CPU-side tests of the C ABI share (test_host_and_abi.py and the test_*_host.py files): where the repository is, the header's
text in the forms they search, and the built binding.  A helper module: no tests in it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1   # DYNENV_ERR_ARG


def header_text():
    """include/dynenv.h as it is"""
    return open(os.path.join(ROOT, "include", "dynenv.h")).read()


def header_without_comments(collapse=True):
    """the header without its /* */ comments and (collapse) every run of white space as one blank, so that a prototype spelled on one
    line is found wherever the header breaks it"""
    txt = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    return re.sub(r"\s+", " ", txt) if collapse else txt


def comment_before(prototype_name):
    """the last comment in front of the declaration of `prototype_name`, white space collapsed"""
    txt = header_text()
    at = re.search(r"^\s*(?:int|void|size_t|const char\s*\*)\s*%s\(" % re.escape(prototype_name), txt, flags=re.M).start()
    return re.sub(r"\s+", " ", txt[:at].rsplit("/*", 1)[1])


def built_capi():
    """dynenv_amd._capi, behind a build of the library it loads (a no-op when the library is newer than its sources)"""
    from dynenv_amd import _capi, build
    build.build()
    return _capi
