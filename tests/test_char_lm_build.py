"""The decode kernels of the character language model (csrc/char_lm.hip) keep their lists in registers: the rows of
docs/vmcnt_audit.md, which tests/test_isa_vmcnt.py holds equal to the built libraries, show no spilled VGPR and no scratch."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows():
    text = open(os.path.join(ROOT, "docs", "vmcnt_audit.md")).read()
    header = next(ln for ln in text.splitlines() if ln.startswith("| kernel |") and "VGPRs spilled" in ln)
    cols = [c.strip() for c in header.strip("|").split("|")]
    rows = {}
    for ln in text.splitlines():
        if re.match(r"\| _Z\w*lm_decode_kernel", ln):
            cells = [c.strip() for c in ln.strip("|").split("|")]
            rows[cells[0]] = dict(zip(cols, cells))
    return rows


def test_both_instantiations_are_listed():
    names = sorted(_rows())
    assert len(names) == 2 and "lm_decode_kernelILi1E" in names[0] and "lm_decode_kernelILi8E" in names[1], names


def test_no_spill_and_no_scratch():
    for name, r in _rows().items():
        assert int(r["VGPRs spilled"]) == 0 and int(r["scratch bytes"]) == 0, (name, r)
        assert r["library"] == "both" and int(r["waivers"]) == 0, (name, r)
