"""The hand-counted `s_waitcnt vmcnt(N)` of every shipped kernel, checked from the disassembly of the built libraries
(tests/isa_vmcnt.py has the model).  No GPU: a stale operand is a timing-dependent failure that a numerical run can miss, while
"this wait covers that load on every feasible path" is a property of the instruction stream.

  a. the model on small hand-written listings (one rule per test; which test guards which rule is in docs/vmcnt_audit.md)
  b. every kernel symbol of libocr_amd.so and libocr_amd_test.so is analysed with every instruction reached, and is clean
  c. seeded defects on the real listings of winograd43_fused<4>, winograd43_x3<4> and conv3x3_bf16_c64 are all reported
  d. register allocation and the statistics of the analysis are recorded in docs/vmcnt_audit.md; a change shows up as a diff

`python -m tests.test_isa_vmcnt` rewrites the table of docs/vmcnt_audit.md from the built libraries.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys

import pytest

from tests import isa_vmcnt as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = {"product": os.path.join(ROOT, "ocr-rs_amd", "lib", "libocr_amd.so"), "test": os.path.join(ROOT, "ocr-rs_amd", "lib", "libocr_amd_test.so")}
AUDIT = os.path.join(ROOT, "docs", "vmcnt_audit.md")

# Kernels of the files with inline-asm loads or hand-written counted waits get the path-sensitive analysis and the non-empty-exec
# assumption (whose justification, with source lines, is in the docstring of tests/isa_vmcnt.py).  Everything else is compiler-only
# code: every branch both ways, no assumption at all - the compiler's own waits hold on every path of the listing.
HAND_COUNTED = re.compile(r"winograd43_fused_kernel|winograd43_x3_kernel|conv_igemm|conv_x3_wide|conv3x3_bf16_c64_kernel|"
                          r"basic_block_bf16_c64_kernel|tail_fused_kernel")

# Waivers: source-level implications between named uniform conditions, for paths the checker cannot prove infeasible.  None is
# needed.  (At most three per kernel source file; never by address, register number or instruction index.)
WAIVERS = {}   # source file -> [{"implication": ..., "source": "file:line"}]
MAX_WAIVERS_PER_FILE = 3

REQUIRED = [   # a renamed or vanished kernel must fail, not shrink the test
    r"winograd43_fused_kernelILi4E", r"winograd43_fused_kernelILi8E", r"winograd43_fused_kernelILi16E",
    r"conv3x3_bf16_c64_kernel", r"basic_block_bf16_c64_kernel",
    r"conv_igemmIffLi\d+ELi\d+ELi\d+ELi\d+ELi0E",          # f32
    r"conv_igemmIffLi\d+ELi\d+ELi\d+ELi\d+ELi[23]E",       # split-bf16 (three / six products)
    r"conv_igemmIDF16bDF16b",                               # bf16
]
TEST_ONLY = [  # the withdrawn kernels (conv_x3w.hip, winograd43_x3.hip): required in the test library, absent from the product library
    r"winograd43_x3_kernelILi4E", r"winograd43_x3_kernelILi8E", r"winograd43_x3_kernelILi16E", r"conv_x3_wide",
]
DELETED = [r"winograd43_out_in_kernel"]   # in neither library


# ---------------------------------------------------------------------------------------------------------------------------
# a. the model on hand-written listings
def _listing(src, name="k", base=0x1000):
    """compact assembly with labels -> the text llvm-objdump -d prints (4 bytes per instruction, branch operands as simm16)"""
    lines = [ln.strip() for ln in src.strip().splitlines() if ln.strip()]
    labels, addr = {}, base
    for ln in lines:
        if ln.endswith(":"):
            labels[ln[:-1]] = addr
        else:
            addr += 4
    out, addr = [f"{base:016x} <{name}>:"], base
    for ln in lines:
        if ln.endswith(":"):
            continue
        mnem, _, ops = ln.partition(" ")
        tail = ""
        if mnem == "s_branch" or mnem.startswith("s_cbranch_"):
            t = labels[ops.strip()]
            ops = str(((t - addr - 4) // 4) & 0xFFFF)
            tail = f" <{name}+{t - base:#x}>"
        out.append(f"\t{mnem} {ops}".ljust(60) + f"// {addr:012X}: BF800000{tail}")
        addr += 4
    return "\n".join(out) + "\n"


def _check(src, **kw):
    return V.analyse(_listing(src), **kw)["k"]


def _hazards(res):
    return [(f.text.split()[0], V.reg_name(f.reg), f.count) for f in res.findings if f.kind == "hazard"]


LOAD_WAIT_USE = """
    buffer_load_dwordx4 v[0:3], v8, s[0:3], 0 offen
    buffer_load_dwordx4 v[4:7], v8, s[0:3], 0 offen offset:16
    s_waitcnt vmcnt({n})
    v_mfma_f32_16x16x4_f32 v[20:23], v9, v0, v[20:23]
    s_waitcnt vmcnt(0)
    v_mov_b32_e32 v10, v4
    s_endpgm
"""


def test_counted_wait_that_covers_its_load_is_clean():
    res = _check(LOAD_WAIT_USE.format(n=1))
    assert res.clean, res.findings
    assert res.tight == {0x1008: 1, 0x1010: 0}     # both waits are exactly as strong as needed
    assert res.stats["queue"] == {"load": 2} and res.stats["waits_counted"] == 1 and res.stats["waits_zero"] == 1


def test_wait_one_too_lenient_is_a_finding_at_the_use():
    res = _check(LOAD_WAIT_USE.format(n=2))
    assert _hazards(res) == [("v_mfma_f32_16x16x4_f32", "v0", 1)]
    f = res.findings[0]
    assert f.addr == 0x100C and "v_mfma" in repr(f) and "v0" in repr(f) and "1 younger" in repr(f)


def test_a_store_between_issue_and_wait_is_a_queue_entry():
    # clean only because the store counts: the load has one younger entry, so vmcnt(1) retires it
    clean = """
        buffer_load_dword v0, v8, s[0:3], 0 offen
        global_store_dword v[12:13], v9, off
        s_waitcnt vmcnt(1)
        v_add_f32_e32 v1, v0, v0
        s_endpgm
    """
    assert _check(clean).clean
    # the same without the store is a finding: nothing but the store's entry makes vmcnt(1) retire the load
    assert _hazards(_check(clean.replace("global_store_dword v[12:13], v9, off", "s_nop 0"))) == [("v_add_f32_e32", "v0", 0)]
    # (the converse - a finding only because a store counts - cannot exist: an entry more only ever raises the numbers, and a wait
    # retires the registers whose number is high enough.)  What a store does add is a finding of its own when it reads a pending register:
    assert _hazards(_check(clean.replace("v9, off", "v0, off"))) == [("global_store_dword", "v0", 0)]
    # ... and an atomic without return counts like a store
    assert _check(clean.replace("global_store_dword v[12:13], v9, off", "global_atomic_add_f32 v[12:13], v9, off")).clean


def test_lds_dma_counts_and_has_no_pending_destination():
    src = """
        buffer_load_dwordx4 v[0:3], v8, s[0:3], 0 offen
        s_mov_b32 m0, s9
        buffer_load_dwordx4 v5, s[4:7], s10 offen lds
        v_mov_b32_e32 v5, 0
        s_waitcnt vmcnt({n})
        v_mov_b32_e32 v6, v0
        s_endpgm
    """
    res = _check(src.format(n=1))       # the DMA is the one younger entry; its address register v5 is free at once
    assert res.clean and res.stats["queue"] == {"load": 1, "lds_dma": 1}
    assert _hazards(_check(src.format(n=2))) == [("v_mov_b32_e32", "v0", 1)]


def test_spill_of_a_pending_register_is_a_finding():
    src = """
        buffer_load_dwordx4 v[0:3], v8, s[0:3], 0 offen
        scratch_store_dwordx4 off, v[0:3], off offset:16
        s_waitcnt vmcnt(0)
        s_endpgm
    """
    assert [h[:2] for h in _hazards(_check(src))] == [("scratch_store_dwordx4", f"v{i}") for i in range(4)]


def test_copy_of_a_pending_register_is_a_finding():
    src = """
        buffer_load_dword v0, v8, s[0:3], 0 offen
        v_mov_b32_e32 v1, v0
        s_waitcnt vmcnt(0)
        s_endpgm
    """
    assert _hazards(_check(src)) == [("v_mov_b32_e32", "v0", 0)]


def test_a_reload_over_a_pending_load_of_another_class_is_a_finding_and_of_the_same_class_is_not():
    src = """
        {first} v[0:1], {addr}
        scratch_load_dword v1, off, off offset:4
        s_waitcnt vmcnt(0)
        v_mov_b32_e32 v2, v1
        s_endpgm
    """
    assert _hazards(_check(src.format(first="buffer_load_dwordx2", addr="v8, s[0:3], 0 offen"))) == [("scratch_load_dword", "v1", 0)]
    # two spill reloads in a row return in order and the younger value wins: the compiler emits this itself
    assert _check(src.format(first="scratch_load_dwordx2", addr="off, off offset:8")).clean


LOOP = """
        buffer_load_dword v0, v8, s[0:3], 0 offen
        s_waitcnt vmcnt(0)
    head:
        v_add_f32_e32 v2, v0, v2
        buffer_load_dword v0, v8, s[0:3], 0 offen
        s_add_i32 s4, s4, -1
        s_cmp_lg_u32 s4, 0
        {wait}
        s_cbranch_scc1 head
        s_waitcnt vmcnt(0)
        s_endpgm
"""


def test_register_pending_across_a_back_edge_is_a_finding_at_the_loop_head():
    assert _hazards(_check(LOOP.format(wait="s_nop 0"))) == [("v_add_f32_e32", "v0", 0)]
    assert _check(LOOP.format(wait="s_waitcnt vmcnt(0)")).clean


def test_join_takes_the_minimum_of_the_counts():
    src = """
        buffer_load_dword v0, v8, s[0:3], 0 offen
        v_cmp_gt_i32_e32 vcc, 0, v9
        s_cbranch_vccz join
        buffer_load_dword v1, v8, s[0:3], 0 offen offset:4
    join:
        s_waitcnt vmcnt(1)
        v_mov_b32_e32 v2, v0
        s_waitcnt vmcnt(0)
        s_endpgm
    """
    # one path leaves v0 with one younger entry (retired by vmcnt(1)), the other with none (not retired): the minimum decides
    assert _hazards(_check(src)) == [("v_mov_b32_e32", "v0", 0)]


# `if (c) issue(); ... if (c) vmcnt(1) else vmcnt(0)` as the compiler writes it: the pair that holds c is overwritten between the
# two tests, which read a copy - the truth belongs to the value, not to the register name
SAME_VALUE_TWICE = """
        s_cmp_lg_u32 s8, 0
        s_cselect_b64 s[10:11], -1, 0
        buffer_load_dword v0, v8, s[0:3], 0 offen
        s_and_b64 vcc, exec, s[10:11]
        s_cbranch_vccz skip
        buffer_load_dword v1, v8, s[0:3], 0 offen offset:4
    skip:
        s_mov_b64 s[12:13], s[10:11]
        s_mov_b64 s[10:11], 0
        s_and_b64 vcc, exec, s[12:13]
        {br} zero
        s_waitcnt vmcnt(1)
        s_branch use
    zero:
        s_waitcnt vmcnt(0)
    use:
        v_mov_b32_e32 v2, v0
        s_waitcnt vmcnt(0)
        s_endpgm
"""
# ... and the threaded form: the first arm leaves -1 / 0 in a pair that the next test branches on
THREADED = """
        s_cmp_lg_u32 s8, 0
        s_cselect_b64 s[10:11], -1, 0
        buffer_load_dword v0, v8, s[0:3], 0 offen
        s_mov_b64 s[12:13], -1
        s_and_b64 vcc, exec, s[10:11]
        s_cbranch_vccz join
        buffer_load_dword v1, v8, s[0:3], 0 offen offset:4
        s_waitcnt vmcnt(1)
        s_mov_b64 s[12:13], 0
    join:
        {test} vcc, exec, s[12:13]
        s_cbranch_vccnz done
        s_waitcnt vmcnt(0)
    done:
        v_mov_b32_e32 v2, v0
        s_waitcnt vmcnt(0)
        s_endpgm
"""


def test_correlated_branches_on_one_value_are_clean_and_inverted_they_are_findings():
    assert _check(SAME_VALUE_TWICE.format(br="s_cbranch_vccz")).clean
    assert _hazards(_check(SAME_VALUE_TWICE.format(br="s_cbranch_vccnz"))) == [("v_mov_b32_e32", "v0", 0)]
    # without conditions every branch goes both ways, and the infeasible path (no second load, the lenient wait) is walked
    assert _hazards(_check(SAME_VALUE_TWICE.format(br="s_cbranch_vccz"), conditions=False)) == [("v_mov_b32_e32", "v0", 0)]


def test_a_pair_overwritten_by_something_unknown_loses_its_truth():
    # between the two tests the pair is reloaded / rewritten by a vector compare: its old truth says nothing about the new value, the
    # second test goes both ways, and the path "no second load, lenient wait" exists again
    for clobber in ("s_load_dwordx2 s[12:13], s[4:5], 0x0", "v_cmp_gt_u32_e64 s[12:13], v9, v8", "s_lshl_b64 s[12:13], s[6:7], 1"):
        src = SAME_VALUE_TWICE.format(br="s_cbranch_vccz").replace("s_mov_b64 s[10:11], 0", clobber)
        assert _hazards(_check(src)) == [("v_mov_b32_e32", "v0", 0)], clobber


def test_threaded_constant_pairs_are_clean_and_inverted_they_are_findings():
    # s[12:13] = -1 means "nothing waited yet": s_andn2 ... vccnz skips the second wait exactly when the first arm ran
    assert _check(THREADED.format(test="s_andn2_b64")).clean
    assert _hazards(_check(THREADED.format(test="s_and_b64"))) == [("v_mov_b32_e32", "v0", 0)]


def test_boolean_algebra_between_conditions():
    # has_patch = !last || next; the wait tests last && !next: two atoms, checked by enumeration
    src = """
        s_cmp_eq_u32 s8, 7
        s_cselect_b64 s[10:11], -1, 0
        s_cmp_lt_i32 s9, s5
        s_cselect_b64 s[12:13], -1, 0
        buffer_load_dword v0, v8, s[0:3], 0 offen
        s_andn2_b64 s[14:15], s[10:11], s[12:13]
        s_not_b64 s[16:17], s[10:11]
        s_or_b64 s[16:17], s[16:17], s[12:13]
        s_and_b64 vcc, exec, s[16:17]
        s_cbranch_vccz nopatch
        buffer_load_dword v1, v8, s[0:3], 0 offen offset:4
    nopatch:
        s_and_b64 vcc, exec, s[14:15]
        s_cbranch_vccnz short
        s_waitcnt vmcnt(1)
        s_branch use
    short:
        s_waitcnt vmcnt(0)
    use:
        v_mov_b32_e32 v2, v0
        s_waitcnt vmcnt(0)
        s_endpgm
    """
    assert _check(src).clean
    assert _hazards(_check(src.replace("s_cbranch_vccnz short", "s_cbranch_vccz short"))) == [("v_mov_b32_e32", "v0", 0)]


def test_condition_through_a_vgpr_keeps_its_truth():
    # hipcc moves a uniform bool through a VGPR: v_cndmask 0 / 1 from the pair, later v_cmp_ne 1 - the pair of the compare is its negation
    src = """
        s_cmp_lg_u64 s[8:9], 0
        s_cselect_b64 s[10:11], -1, 0
        v_cndmask_b32_e64 v3, 0, 1, s[10:11]
        v_cmp_ne_u32_e64 s[12:13], 1, v3
        s_and_b64 vcc, exec, s[12:13]
        s_cbranch_vccnz noload
        buffer_load_dword v0, v8, s[0:3], 0 offen
    noload:
        s_and_b64 vcc, exec, s[10:11]
        s_cbranch_vccz nowait
        s_waitcnt vmcnt(0)
    nowait:
        s_and_b64 vcc, exec, s[12:13]
        s_cbranch_vccnz end
        v_mov_b32_e32 v2, v0
    end:
        s_endpgm
    """
    assert _check(src).clean
    assert _hazards(_check(src.replace("v_cmp_ne_u32_e64", "v_cmp_eq_u32_e64"))) != []


TRIP_COUNT = """
        v_readfirstlane_b32 s3, v0
        s_lshr_b32 s7, s3, 6
        buffer_load_dword v1, v8, s[0:3], 0 offen
        s_add_i32 s9, s7, -4
    loop:
        buffer_load_dwordx4 v5, s[4:7], s10 offen lds
        s_add_i32 s9, s9, 4
        s_cmp_lt_u32 s9, 19
        s_cbranch_scc1 loop
        s_waitcnt vmcnt({n})
        v_mov_b32_e32 v2, v1
        s_waitcnt vmcnt(0)
        s_endpgm
"""


def test_work_item_id_range_decides_a_trip_count():
    # `for (k = wave; k < 23; k += 4) dma()` with wave = tid >> 6: five or six DMAs when the workgroup has at most 256 work-items
    res = _check(TRIP_COUNT.format(n=5), max_workgroup=256)
    assert res.clean and res.tight[0x1020] == 5
    assert _hazards(_check(TRIP_COUNT.format(n=6), max_workgroup=256)) == [("v_mov_b32_e32", "v1", 5)]
    # without the bound the loop may leave after one DMA; with 1024 work-items (wave < 16) after two
    assert _hazards(_check(TRIP_COUNT.format(n=5))) == [("v_mov_b32_e32", "v1", 1)]
    assert _hazards(_check(TRIP_COUNT.format(n=5), max_workgroup=1024)) == [("v_mov_b32_e32", "v1", 2)]
    # and v0 must still be what the kernel was entered with
    assert _hazards(_check(TRIP_COUNT.format(n=5).replace("v_readfirstlane_b32 s3, v0", "v_mov_b32_e32 v0, v9\n v_readfirstlane_b32 s3, v0"),
                           max_workgroup=256)) == [("v_mov_b32_e32", "v1", 1)]


EXEC_SKIP = """
        buffer_load_dword v0, v8, s[0:3], 0 offen
        v_cmp_gt_u32_e32 vcc, 8, v9
        s_and_saveexec_b64 s[4:5], vcc
        s_cbranch_execz skip
        buffer_load_dwordx4 v5, s[4:7], s10 offen lds
    skip:
        s_or_b64 exec, exec, s[4:5]
        s_waitcnt vmcnt(1)
        v_mov_b32_e32 v2, v0
        s_waitcnt vmcnt(0)
        s_endpgm
"""


def test_exec_skip_around_a_load_under_the_assumption_and_without_it():
    res = _check(EXEC_SKIP)
    assert res.clean and res.stats["skipped_by_exec_assumption"] == 0
    assert _hazards(_check(EXEC_SKIP, nonempty_exec=False)) == [("v_mov_b32_e32", "v0", 0)]


def test_divergent_loop_back_edge_goes_both_ways_under_the_assumption():
    src = """
    head:
        v_cmp_gt_u32_e32 vcc, v1, v9
        s_andn2_b64 exec, exec, vcc
        s_cbranch_execnz head
        s_mov_b64 exec, s[4:5]
        s_endpgm
    """
    assert _check(src).clean      # the exit is reached: a loop's exec test is not a region guard


def test_unreachable_unknown_control_flow_and_unknown_instruction_classes_are_findings():
    kinds = lambda res: sorted({f.kind for f in res.findings})
    assert kinds(_check("s_branch end\n v_mov_b32_e32 v0, v1\n end:\n s_endpgm")) == ["unreachable instruction"]
    assert kinds(_check("s_getpc_b64 s[0:1]\n s_setpc_b64 s[0:1]\n s_endpgm")) == ["unknown control flow", "unreachable instruction"]
    assert kinds(_check("s_swappc_b64 s[30:31], s[0:1]\n s_endpgm")) == ["unknown control flow", "unreachable instruction"]
    # a scalar mnemonic outside the table of known ones (which is how a scalar memory write would show up) ...
    assert kinds(_check("s_frobnicate_dword s0, s[2:3], 0x0\n s_endpgm")) == ["unknown scalar instruction"]
    # ... a vector-memory instruction that is neither load, store nor atomic, and a class the model has no place for
    assert kinds(_check("buffer_frob_dword v0, v1, s[0:3], 0 offen\n s_endpgm")) == ["unknown vector-memory instruction"]
    assert kinds(_check("image_sample v[0:3], v[4:5], s[0:7], s[8:11] dmask:0xf\n s_endpgm")) == ["unknown instruction class"]
    assert kinds(_check("v_mov_b32_e32 v0, v1")) == ["control runs off the end of the function"]


# ---------------------------------------------------------------------------------------------------------------------------
# b - d. the built libraries
def _tool(name):
    for d in ["/opt/rocm/llvm/bin"] + os.environ.get("PATH", "").split(os.pathsep):
        p = os.path.join(d, name)
        if os.path.isfile(p) and os.access(p, os.X_OK):
            return p
    pytest.fail(f"{name} not found (looked in /opt/rocm/llvm/bin and PATH): the vmcnt check needs the ROCm LLVM tools - a hazard "
                "check that is skipped hides exactly what it is for")


def _run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(f"{' '.join(cmd)} failed: {r.stderr[-400:]}")
    return r.stdout


def _metadata(notes):
    """llvm-readelf --notes of a code object -> {kernel: {vgpr, agpr, spill, scratch}}"""
    out = {}
    for blk in re.split(r"(?m)^  - (?=\.)", notes)[1:]:
        get = lambda k: (re.search(r"(?m)^\s+\.%s:\s+(\S+)" % k, "    " + blk) or [None, None])[1]
        name = get("name")
        if name is not None and get("vgpr_count") is not None:
            out[name] = {"vgpr": int(get("vgpr_count")), "agpr": int(get("agpr_count") or 0), "spill": int(get("vgpr_spill_count")),
                         "scratch": int(get("private_segment_fixed_size")), "wg": int(get("max_flat_workgroup_size") or 0)}
    return out


def extract(lib, workdir):
    """the gfx950 code objects of a built library -> ({kernel: listing text of that function}, {kernel: metadata}, compiler)"""
    if not os.path.exists(lib):
        pytest.fail(f"{lib} is missing: run __graft_entry__.build() first")
    os.makedirs(workdir, exist_ok=True)
    so = os.path.join(workdir, "lib.so")
    shutil.copy(lib, so)
    objdump, readelf = _tool("llvm-objdump"), _tool("llvm-readelf")
    _run([objdump, "--offloading", "lib.so"], workdir)
    objs = sorted(f for f in os.listdir(workdir) if f.startswith("lib.so.") and "gfx950" in f)
    if not objs:
        pytest.fail(f"no gfx950 code object in {lib}")
    text, meta, compiler = {}, {}, set()
    for o in objs:
        listing = _run([objdump, "-d", o], workdir)
        for name, lines in V.split_functions(listing).items():
            text[name] = "\n".join(lines) + "\n"
        meta.update(_metadata(_run([readelf, "--notes", o], workdir)))
        compiler.update(re.findall(r"(?:AMD )?clang version [^\n\]]*", _run([readelf, "-p", ".comment", o], workdir)))
    return text, meta, sorted(compiler)


_CACHE = {}


def audit(workdir):
    """both libraries extracted and every kernel analysed, once per session"""
    if "rows" in _CACHE:
        return _CACHE
    libs = {k: extract(p, os.path.join(workdir, k)) for k, p in LIBS.items()}
    rows, results, texts = [], {}, {}
    for which, (text, meta, _) in libs.items():
        for name in sorted(text):
            stream = [ln.split("//")[0].strip() for ln in text[name].splitlines()[1:]]   # (branch operands are relative)
            if name in results and texts[name][1] == stream:
                for r in rows:
                    if r["kernel"] == name:
                        r["library"] = "both"
                continue
            key = name if name not in results else name + " (test library)"
            full = bool(HAND_COUNTED.search(name))
            res = V.analyse(text[name], nonempty_exec=full, conditions=full, max_workgroup=((meta.get(name) or {}).get("wg") or None) if full else None)[name]
            results[key], texts[key] = res, (text[name], stream)
            _CACHE.setdefault("wg", {})[key] = ((meta.get(name) or {}).get("wg") or None) if full else None
            # mnemonics and operands without addresses and encodings (branch operands are relative): two builds have the same
            # hash exactly when the compiler emitted the same instructions for the kernel
            sha = hashlib.sha256("\n".join(stream).encode()).hexdigest()[:12]
            rows.append({"stream_sha": sha, "kernel": key, "library": which, "analysis": "path-sensitive" if full else "both ways", "meta": meta.get(name), "res": res})
    _CACHE.update(rows=rows, results=results, texts=texts, compiler=sorted({c for _, _, cs in libs.values() for c in cs}),
                  symbols={k: set(v[0]) for k, v in libs.items()}, kernels={k: set(v[1]) for k, v in libs.items()})
    return _CACHE


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return audit(str(tmp_path_factory.mktemp("vmcnt")))


COLUMNS = ["kernel", "library", "analysis", "VGPRs", "AGPRs", "VGPRs spilled", "scratch bytes", "instructions", "loads", "LDS-DMA", "stores",
           "atomics", "vmcnt(0) waits", "counted waits", "tight waits", "tight counted waits", "not reached by the path-sensitive analysis", "peak states",
           "waivers", "instruction stream", "seconds"]


KERNEL_FILES = {   # kernel symbol -> its source file, for the files that may carry waivers
    r"winograd43_fused_kernel": "winograd43_fused.hip", r"winograd43_x3_kernel": "winograd43_x3.hip", r"conv_igemm": "conv_igemm.hip",
    r"conv_x3_wide": "conv_x3w.hip", r"conv3x3_bf16_c64_kernel": "conv3x3_bf16_c64.hip",
    r"basic_block_bf16_c64_kernel": "basic_block_bf16_c64.hip", r"tail_fused_kernel": "tail_fused.hip",
}


def _waivers_of(kernel):
    return sum(len(WAIVERS.get(f, [])) for pat, f in KERNEL_FILES.items() if re.search(pat, kernel))


def table_rows(rows):
    out = []
    for r in rows:
        s, m = r["res"].stats, r["meta"] or {}
        q = s["queue"]
        out.append([r["kernel"], r["library"], r["analysis"], m.get("vgpr", "?"), m.get("agpr", "?"), m.get("spill", "?"), m.get("scratch", "?"),
                    s["instructions"], q.get("load", 0), q.get("lds_dma", 0), q.get("store", 0), q.get("atomic", 0), s["waits_zero"],
                    s["waits_counted"], s["tight"], s["tight_counted"], s["skipped_by_exec_assumption"], s["peak_states"], _waivers_of(r["kernel"]),
                    r["stream_sha"], "%.2f" % s["seconds"]])
    return [[str(c) for c in row] for row in out]


def render_table(rows):
    lines = ["| " + " | ".join(COLUMNS) + " |", "|" + "---|" * len(COLUMNS)]
    return "\n".join(lines + ["| " + " | ".join(r) + " |" for r in table_rows(rows)]) + "\n"


def committed_table():
    if not os.path.exists(AUDIT):
        pytest.fail("docs/vmcnt_audit.md is missing")
    doc = open(AUDIT).read()
    m = re.search(r"<!-- table:begin -->\n(.*?)<!-- table:end -->", doc, re.S)
    if not m:
        pytest.fail("docs/vmcnt_audit.md has no table between its markers")
    return [[c.strip() for c in ln.strip().strip("|").split("|")] for ln in m.group(1).strip().splitlines()[2:]]


def _committed_kernels():
    try:
        return [r[0] for r in committed_table()]
    except BaseException:    # reported by test_the_audit_file_lists_exactly_the_kernels_of_the_libraries
        return []


def test_every_launch_of_a_hand_counted_kernel_is_one_dimensional():
    """the range of the work-item id (tests/isa_vmcnt.py, "Value ranges") rests on v0 being the flat id: every launch of a kernel of
    the hand-counted files must pass a one-dimensional block"""
    csrc = os.path.join(ROOT, "ocr-rs_amd", "csrc")
    seen = 0
    for f in sorted(set(KERNEL_FILES.values())):
        src = open(os.path.join(csrc, f)).read()
        for m in re.finditer(r"hipLaunchKernelGGL\((.*?)\);", src, re.S):
            args = m.group(1)
            blocks = []
            for d in re.finditer(r"dim3\(", args):     # the balanced argument list of every dim3(...)
                depth, j = 1, d.end()
                while depth:
                    depth += {"(": 1, ")": -1}.get(args[j], 0)
                    j += 1
                blocks.append(args[d.end():j - 1])
            blocks = [b for k, b in enumerate(blocks) if not any(b in o and b != o for o in blocks)]   # (a dim3 inside a dim3: none)
            assert len(blocks) == 2, (f, args[:80])
            assert "," not in re.sub(r"\([^()]*\)", "", blocks[1]), f"{f}: block {blocks[1]!r} is not one-dimensional"
            seen += 1
        assert "<<<" not in src, f
    assert seen >= 7


def test_waivers_are_within_the_cap_and_cite_their_source():
    for f, ws in WAIVERS.items():
        assert len(ws) <= MAX_WAIVERS_PER_FILE, f
        for w in ws:
            assert re.match(r".+\.hip:\d+", w["source"]) and "=>" in w["implication"]


def test_the_audit_file_lists_exactly_the_kernels_of_the_libraries(built):
    """the kernels below are parametrised from the committed audit table (it exists before anything is built): a kernel that the
    libraries have and the table has not, or the reverse, fails here"""
    analysed = [r["kernel"] for r in built["rows"]]
    assert analysed, "no kernel symbol found in the libraries"
    for which in LIBS:
        assert built["symbols"][which] == built["kernels"][which], f"{which}: function symbols and metadata kernels differ"
    assert built["symbols"]["product"] <= built["symbols"]["test"]
    for pat in REQUIRED:
        for which in LIBS:
            assert any(re.search(pat, n) for n in built["symbols"][which]), f"no kernel matching {pat} in the {which} library"
    for pat in TEST_ONLY:
        assert any(re.search(pat, n) for n in built["symbols"]["test"]), f"no kernel matching {pat} in the test library"
        assert not any(re.search(pat, n) for n in built["symbols"]["product"]), f"a kernel matching {pat} in the product library"
    for pat in DELETED:
        for which in LIBS:
            assert not any(re.search(pat, n) for n in built["symbols"][which]), f"a kernel matching {pat} in the {which} library"
    assert sorted(analysed) == sorted(_committed_kernels()), "docs/vmcnt_audit.md is out of date: python -m tests.test_isa_vmcnt"


@pytest.mark.parametrize("kernel", _committed_kernels() or ["<docs/vmcnt_audit.md has no kernels>"])
def test_shipped_kernel_is_clean(built, kernel):
    """every kernel of both libraries, every instruction reached, no finding"""
    assert kernel in built["results"], f"{kernel}: listed in docs/vmcnt_audit.md, not in the libraries"
    res = built["results"][kernel]
    assert res.stats["instructions"] > 0
    assert res.clean, f"{kernel}: {len(res.findings)} findings\n" + "\n".join(repr(f) for f in res.findings[:12])


def test_allocation_and_statistics_match_the_committed_audit(built):
    """everything but the seconds: a compiler or source change that moves the allocation (VGPRs, spills, scratch) or the instruction
    stream shows up here as a diff to look at and re-commit (python -m tests.test_isa_vmcnt), with the hazard analysis green"""
    want = {r[0]: r[:-1] for r in committed_table()}
    got = {r[0]: r[:-1] for r in table_rows(built["rows"])}
    diff = [f"{k}:\n   committed {want.get(k)}\n   built     {got.get(k)}" for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)]
    assert not diff, "docs/vmcnt_audit.md differs from the built libraries:\n" + "\n".join(diff[:10])
    fused = [r for r in built["rows"] if "winograd43_fused_kernel" in r["kernel"]]
    assert len(fused) == 3 and all(r["meta"]["vgpr"] == 255 and r["meta"]["spill"] == 4 for r in fused)   # what DESIGN 3.4 states


# ---------------------------------------------------------------------------------------------------------------------------
# c. seeded defects on the real listings
SEEDED = {   # kernel -> the hand-written counted waits of its matrix phase that must come out tight (source lines in the ids)
    "winograd43_fused_kernelILi4E": 12,    # winograd43_fused.hip:324-335, twelve steps per chunk body
    "winograd43_x3_kernelILi4E": 9,        # winograd43_x3.hip:327-333, nine steps per chunk
    "conv3x3_bf16_c64_kernel": 1,          # conv3x3_bf16_c64.hip: vmcnt(5) before the store phase
}


def _kernel(built, pat):
    names = [k for k in built["results"] if re.search(pat, k)]
    assert len(names) == 1, (pat, names)
    return names[0], built["texts"][names[0]][0].splitlines()


def _analyse_lines(name, lines):
    return V.analyse("\n".join(lines) + "\n", max_workgroup=_CACHE["wg"][name])[name]


def _new_hazards(base, mutant):
    """hazards of the mutated listing that the shipped listing does not have (same instruction, same register)"""
    known = {(f.addr, f.reg) for f in base.findings if f.kind == "hazard"}
    return [f for f in mutant.findings if f.kind == "hazard" and (f.addr, f.reg) not in known]


def _line_of(lines, addr):
    hits = [i for i, ln in enumerate(lines) if re.search(r"//\s*0*%X:" % addr, ln)]
    assert len(hits) == 1, hex(addr)
    return hits[0]


@pytest.mark.parametrize("pat", sorted(SEEDED))
def test_every_tight_wait_made_one_more_lenient_is_reported(built, pat):
    name, lines = _kernel(built, pat)
    base = built["results"][name]
    assert base.stats["tight_counted"] >= SEEDED[pat], "a checker that finds no counted wait tight is not looking"
    missed = []
    for addr, n in sorted(base.tight.items()):
        i = _line_of(lines, addr)
        assert f"vmcnt({n})" in lines[i]
        mutant = _analyse_lines(name, lines[:i] + [lines[i].replace(f"vmcnt({n})", f"vmcnt({n + 1})")] + lines[i + 1:])
        if not _new_hazards(base, mutant):
            missed.append(f"{addr:#x}: vmcnt({n}) -> vmcnt({n + 1})")
    assert not missed, f"{name}: {len(missed)} of {len(base.tight)} weakened waits not reported: {missed}"


def _first_register_load(lines):
    for i, ln in enumerate(lines):
        m = re.match(r"\s+buffer_load_dwordx4 (v\[\d+:\d+\]), .*offen\s*//\s*([0-9A-F]+):", ln)
        if m and " lds" not in ln:
            return i, m.group(1), int(m.group(2), 16)
    raise AssertionError("no buffer_load_dwordx4 into registers")


@pytest.mark.parametrize("pat", sorted(SEEDED))
@pytest.mark.parametrize("what", ["spill", "reload"])
def test_spill_or_reload_of_a_ring_register_after_its_load_is_reported(built, pat, what):
    name, lines = _kernel(built, pat)
    i, reg, addr = _first_register_load(lines)
    ins = f"scratch_store_dwordx4 off, {reg}, off offset:16" if what == "spill" else f"scratch_load_dwordx4 {reg}, off, off offset:16"
    mutant = lines[:i + 1] + [f"\t{ins}".ljust(60) + f"// {addr + 4:012X}: DC000000"] + lines[i + 1:]
    found = [f for f in _new_hazards(built["results"][name], _analyse_lines(name, mutant)) if f.addr == addr + 4]
    assert found, f"{name}: {ins} after the load at {addr:#x} not reported"


@pytest.mark.parametrize("pat", sorted(SEEDED))
def test_a_deleted_counted_wait_is_reported(built, pat):
    name, lines = _kernel(built, pat)
    base = built["results"][name]
    counted = [a for a, n in sorted(base.tight.items()) if n > 0]
    assert counted
    # (the last counted waits of the listing: in all three kernels those are hand-written ones - the compiler's own counted waits in
    # front of a stronger hand-written wait are not needed, see the weakening test)
    for addr in counted[-3:]:
        i = _line_of(lines, addr)
        res = _analyse_lines(name, lines[:i] + [re.sub(r"s_waitcnt vmcnt\(\d+\)( lgkmcnt\(\d+\))?", lambda m: "s_nop 0" + " " * (len(m.group(0)) - 7), lines[i])] + lines[i + 1:])
        assert _new_hazards(base, res), f"{name}: wait at {addr:#x} deleted, nothing reported"


def test_the_frozen_kernel_has_one_shape_in_its_three_instantiations():
    """winograd43_fused_kernel<4|8|16> differ in the trip count of the chunk loop only: the same instruction counts, waits and allocation.
    Together with the table comparison above, an edit of the frozen file that was meant to touch comments only and moved an
    instruction or a spill fails."""
    rows = {r[0]: r for r in committed_table() if "winograd43_fused_kernel" in r[0]}
    assert len(rows) == 3 and len({tuple(r[3:-2]) for r in rows.values()}) == 1     # (all but the stream hash and the seconds)


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        a = audit(d)
    doc = open(AUDIT).read() if os.path.exists(AUDIT) else "<!-- table:begin -->\n<!-- table:end -->\n"
    doc = re.sub(r"<!-- table:begin -->\n.*?<!-- table:end -->", lambda m: "<!-- table:begin -->\n" + render_table(a["rows"]) + "<!-- table:end -->", doc, flags=re.S)
    open(AUDIT, "w").write(doc)
    bad = {k: len(r.findings) for k, r in a["results"].items() if not r.clean}
    print(f"{len(a['rows'])} kernels, compiler {a['compiler']}, {sum(r['res'].stats['seconds'] for r in a['rows']):.1f} s; not clean: {bad}", file=sys.stderr)
