"""The kernels of the segmentation lattice (csrc/lattice.hip, csrc/glyph_split.hip) keep their lists and cuts in registers: the rows of
docs/vmcnt_audit.md, which tests/test_isa_vmcnt.py holds equal to the built libraries, show no spilled VGPR and no scratch; and the
header's new calls are what the wrapper binds."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(pattern):
    text = open(os.path.join(ROOT, "docs", "vmcnt_audit.md")).read()
    header = next(ln for ln in text.splitlines() if ln.startswith("| kernel |") and "VGPRs spilled" in ln)
    cols = [c.strip() for c in header.strip("|").split("|")]
    rows = {}
    for ln in text.splitlines():
        if re.match(pattern, ln):
            cells = [c.strip() for c in ln.strip("|").split("|")]
            rows[cells[0]] = dict(zip(cols, cells))
    return rows


def _kernels():
    rows = _rows(r"\| _Z\w*lattice_decode_kernel")
    rows.update(_rows(r"\| _Z\w*12split_kernel"))
    return rows


def test_both_decode_instantiations_and_the_split_kernel_are_listed():
    names = sorted(_kernels())
    assert len(names) == 3, names
    assert "split_kernel" in names[0] and "lattice_decode_kernelILi1E" in names[1] and "lattice_decode_kernelILi8E" in names[2], names


def test_no_spill_no_scratch_no_waiver():
    for name, r in _kernels().items():
        assert int(r["VGPRs spilled"]) == 0 and int(r["scratch bytes"]) == 0, (name, r)
        assert r["library"] == "both" and int(r["waivers"]) == 0, (name, r)


def test_the_header_declares_what_the_wrapper_binds():
    from ocr_rs_amd import capi
    header = open(os.path.join(ROOT, "include", "ocr_amd.h")).read()
    for name in ("ocr_split_default_params", "ocr_split_glyphs", "ocr_piece_map_free", "ocr_glyph_spans", "ocr_span_table_free",
                 "ocr_lattice_default_params", "ocr_lattice_decode", "ocr_lattice_paths_free"):
        assert re.search(r"\b%s\(" % name, header) and name in capi.EXPORTS, name
    assert "#define OCR_LATTICE_MAX_SPAN 4" in header and "#define OCR_LATTICE_MAX_PIECES 32" in header
    assert capi.LATTICE_MAX_SPAN == 4 and capi.LATTICE_MAX_PIECES == 32
