"""The kernels of the joint lexicon and lattice search (csrc/lexicon_lattice.hip) keep the DP column and the best-k in registers: the
rows of docs/vmcnt_audit.md, which tests/test_isa_vmcnt.py holds equal to the built libraries, show no spilled VGPR and no scratch in
any instantiation; the header's new calls are what the wrapper binds; and the host side (csrc/lexicon_lattice_host.cpp: parameter
check, offsets check, per-word plan) passes the checks of its stand-alone program."""
import os
import re
import subprocess

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


def test_every_kernel_and_instantiation_is_listed():
    names = sorted(_rows(r"\| _Z\w*lexlat_\w+_kernel"))
    assert len(names) == 19, names
    assert sum("lexlat_raw_kernel" in n for n in names) == 1 and sum("lexlat_merge_kernel" in n for n in names) == 1
    assert sum("lexlat_trace_kernel" in n for n in names) == 1
    for k in (1, 8):                 # best-k of 1 or 8
        for m in (1, 2, 3, 4):       # max_span
            for z in (0, 1):         # with the span costs' adds, and without them for a call whose span costs are all zero
                assert sum("lexlat_match_kernelILi%dELi%dELb%dEE" % (k, m, z) in n for n in names) == 1, (k, m, z)


def test_no_spill_no_scratch_no_waiver():
    for name, r in _rows(r"\| _Z\w*lexlat_\w+_kernel").items():
        assert int(r["VGPRs spilled"]) == 0 and int(r["scratch bytes"]) == 0, (name, r)
        assert r["library"] == "both" and int(r["waivers"]) == 0, (name, r)


def test_the_lexicon_kernels_are_listed_as_before():
    names = sorted(_rows(r"\| _Z\w*(lex_raw|lex_match|lex_merge|glyph_cost)_kernel"))
    assert len(names) == 5, names


def test_the_header_declares_what_the_wrapper_binds():
    from ocr_rs_amd import capi
    header = open(os.path.join(ROOT, "include", "ocr_amd.h")).read()
    for name in ("ocr_lexlat_default_params", "ocr_lexicon_lattice_match", "ocr_lexlat_matches_free"):
        assert re.search(r"\b%s\(" % name, header) and name in capi.EXPORTS, name
    for field in ("ins_cost", "del_cost", "span_cost[4]", "max_span", "max_len_diff", "fold_case", "top_k", "reserved[2]"):
        assert re.search(r"typedef struct ocr_lexlat_params \{[^}]*\b%s;" % re.escape(field), header), field
    assert [f for f, _ in capi.LexLatParams._fields_] == ["ins_cost", "del_cost", "span_cost", "max_span", "max_len_diff", "fold_case",
                                                          "top_k", "reserved"]
    assert [f for f, _ in capi.LexLatMatchesBlock._fields_] == ["n_words", "top_k", "n_pieces", "entries", "costs", "raw_costs",
                                                                "n_candidates", "word_flags", "seg_len", "seg_char", "n_ins"]
    for f, _ in capi.LexLatMatchesBlock._fields_[3:]:
        assert re.search(r"typedef struct ocr_lexlat_matches \{[^}]*\b%s;" % f, header), f
    p = capi.lexlat_params()
    assert (p.ins_cost, p.del_cost, list(p.span_cost), p.max_span, p.max_len_diff, p.fold_case, p.top_k, list(p.reserved)) == \
        (4.0, 4.0, [0.0] * 4, 2, 2, 1, 1, [0, 0])
    assert hasattr(capi.Recognizer, "lexicon_lattice_match") and hasattr(capi.Recognizer, "lexicon_lattice_match_device")
    assert hasattr(capi.LexLatMatches, "segments")


def test_host_plan_through_its_stand_alone_program(tmp_path):
    """tools/fuzz/lexicon_lattice_host_fuzz.cpp checks the plan against its definition (rows, flags, the candidate range counted entry
    by entry under the length rule) and every broken input for a refusal; here it is built plainly and run for 300 rounds."""
    exe = str(tmp_path / "lexicon_lattice_host_fuzz")
    csrc = os.path.join(ROOT, "ocr-rs_amd", "csrc")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "fuzz", "lexicon_lattice_host_fuzz.cpp"), os.path.join(csrc, "lexicon_lattice_host.cpp"),
                    os.path.join(csrc, "lexicon_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, "300"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.match(r"300 plans, \d+ candidates, \d+ refused", out.stdout), out.stdout
