"""engine_cases.ROUTE_KNOBS, which every GPU test's engine builder clears, is the set of names the C sources read from the environment."""
import glob
import os
import re

from conftest import ROOT
from engine_cases import ROUTE_KNOBS


def test_route_knobs_are_the_names_the_sources_read():
    """Every string literal that opens a getenv argument under csrc/: whole names, and the two prefixes completed at run time
    (SE_CONVP_NT_<plan>, SE_DEC_PAIR_dec<j>).  A knob added to the sources fails here until ROUTE_KNOBS has it."""
    read = set()
    for path in glob.glob(os.path.join(ROOT, "speech_enhancement_mi_amd", "csrc", "*")):
        if os.path.isfile(path) and path.endswith((".h", ".hip", ".cpp", ".c", ".inc")):
            read |= set(re.findall(r'\bgetenv\s*\(\s*\(?\s*"([^"]*)"', open(path, errors="replace").read()))
    assert {"SE_PIPELINE", "SE_CONVP_NT_", "SE_DEC_PAIR_dec", "SE_FSN_PIPELINE"} <= read, sorted(read)
    assert read == ROUTE_KNOBS, (sorted(read - ROUTE_KNOBS), sorted(ROUTE_KNOBS - read))
