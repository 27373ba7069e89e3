"""INTEGRATION.md's paragraph of environment switches lists exactly the MA_* variables the library reads (MA_LIB belongs to
the Python binding): a switch added to or retired from lancet2_amd/csrc without the document fails here."""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_integration_lists_exactly_the_switches_the_library_reads():
    read = set()
    for path in glob.glob(os.path.join(REPO, "lancet2_amd", "csrc", "*.hip")) + glob.glob(os.path.join(REPO, "lancet2_amd", "csrc", "*.h")):
        read |= set(re.findall(r'getenv\("(MA_\w+)"\)', open(path).read()))
    doc = open(os.path.join(REPO, "INTEGRATION.md")).read()
    para = doc[doc.index("Environment switches read by the library"):]
    para = para[:para.index("\n## ")]
    listed = set(re.findall(r"`(MA_\w+)`", para)) - {"MA_LIB"}
    assert read, "no getenv(\"MA_...\") found under lancet2_amd/csrc"
    assert read - listed == set(), "read by the library, missing from INTEGRATION.md: %s" % sorted(read - listed)
    assert listed - read == set(), "listed in INTEGRATION.md, not read by the library: %s" % sorted(listed - read)
