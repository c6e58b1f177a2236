"""Static check of `s_waitcnt vmcnt(N)` against the instruction stream of a gfx950 code object.

Input is the text `llvm-objdump -d` prints for a code object; output is, per function symbol, a list of findings and a
statistics record.  Nothing here runs on a GPU and nothing is numerical: whether a wait covers the load it is meant for is a
property of the instruction stream, so it is decided from the instruction stream.

Model (gfx9 / CDNA: one counter for every vector-memory operation)
  * every vector-memory instruction (buffer_ / global_ / scratch_ / flat_ / tbuffer_: loads, stores, atomics, LDS-DMA loads
    with the `lds` modifier) enters the wave's VM queue in program order;
  * `s_waitcnt vmcnt(N)` (alone or with other counters) leaves at most the N youngest entries outstanding;
  * a load without `lds` (and an atomic that returns) marks its destination VGPRs *pending* until it is retired; an LDS-DMA
    load and a store count in the queue and have no pending destination;
  * for every pending register the state keeps the LEAST number of younger queue entries over all feasible paths to the
    program point, so `vmcnt(N)` retires exactly the registers whose number is >= N; a join takes the union of the registers
    and the minimum of the numbers; the numbers saturate at 64 (vmcnt has six bits), which makes the state space finite;
  * FINDING: an instruction that names a pending VGPR / AGPR, as source or as destination (an MFMA operand, a v_mov, a spill
    store, an address, a load of another class into the register).  Exit and back edges need no rule: pending registers flow
    along edges.  One exception, because the compiler itself emits it (a reload hoisted above a branch, a wide reload followed by a
    narrow one): a load whose DESTINATION is pending from a load of the same class (scratch / global / buffer) is not reported -
    loads of one class return in order and the younger value wins.  A scratch reload over an inline-asm buffer load is reported.

Control flow is rebuilt from s_branch / s_cbranch_* / s_endpgm.  Every instruction of a function must be reached; an
unreached instruction, any other control transfer (s_setpc_b64, s_swappc_b64, calls, forks, traps), an s_* mnemonic that is
not in the table of known scalar instructions (which is how scalar memory writes are caught without being spelled here) and
any instruction of an unknown class are findings of their own.

Feasibility.  Taking every branch both ways walks paths that cannot happen (`if (has_patch) vmcnt(18) else vmcnt(9)` behind
`if (has_patch) issue_patch()`), so uniform conditions are tracked as boolean functions (a small BDD) over atoms:
  * an atom is the truth of one scalar comparison, keyed by the VALUES compared (s_cmp_* / s_cmpk_* / s_bitcmp*; the values
    of SGPRs are numbered where they are first read and follow s_mov_b32 / s_mov_b64), or of an SCC the checker did not see
    being set, keyed by the instruction that reads it;
  * SGPR pairs hold such functions when they are produced by `s_cselect_b64 -1, 0`, `s_mov_b64 -1 / 0`, pair-to-pair
    s_mov_b64 and s_and / s_or / s_xor / s_andn2 / s_orn2 / s_nand / s_nor / s_xnor / s_not _b64 of such pairs; vcc from
    `s_and_b64 / s_andn2_b64 vcc, exec, pair`; a function belongs to the value, not to the register name;
  * hipcc also moves a uniform condition through a VGPR (`v_cndmask_b32 v, 0, 1, pair` ... `v_cmp_ne_u32 pair', 1, v`): the
    function follows, as long as exec is the value it was at the select (exec values are numbered where they are written;
    `s_or_b64 exec, exec, saved` restores the number the saveexec saw);
  * a pair written by anything else (v_cmp lane masks, loads) is a lane mask the checker knows nothing about.  It carries no
    assumption of uniformity; what is tracked is only that `exec & mask` (or `exec & ~mask`) tested twice on the same value of the
    mask and of exec has the same answer twice; `s_not_b64` / `s_xor_b64 .., -1` of such a mask is its complement;
  * a path carries the conjunction of what its branches assumed; a branch whose condition contradicts it is not taken.  The
    assumption is forgotten (existentially quantified) once no register, condition code or still-comparable value holds its atoms;
  * states at a block entry are folded into one when their pending registers agree and nothing is forgotten by it (the
    conditions become `if-then-else` on the assumptions that told the states apart, which is exact) or when their conditions agree
    (minimum of the numbers); beyond `max_states` per entry everything is folded, which forgets conditions but never a path.

The first of two global assumptions, `nonempty_exec` (on by default): a region the compiler guards with `s_*_saveexec_b64` followed by
`s_cbranch_execz` (skip) or `s_cbranch_execnz` (enter an out-of-line body) is entered by at least one lane of every wave.  Any
other branch on exec - the back edge or the exit of a divergent loop, which ends exactly when no lane is left - goes both ways.
The regions that issue counted loads in this project are entered by construction:
ocr-rs_amd/csrc/winograd43_fused.hip:206 and winograd43_x3.hip:227 (patch DMA under `part == 0 || lane < 8`: waves with
part == 1 keep lanes 0-7; a wave-uniform "off" is a separate scalar branch that the checker follows as a condition),
conv3x3_bf16_c64.hip:111 and basic_block_bf16_c64.hip (DMA unconditional per wave).  With the assumption off, a load inside
such a region is counted on one path and not on the other, and every older load's number drops.  What the assumption cuts off
(the path on which the region is skipped) is not hazard-checked; those instructions are still walked once, every branch both
ways, so that no instruction of a kernel goes unread (statistics: skipped_by_exec_assumption, which also counts what the condition reasoning itself proves dead).  The test applies the assumption
to the kernels of the seven hand-counted files only; compiler-only kernels are analysed with every branch both ways.

A second assumption, value ranges, when the caller passes the code object's `.max_flat_workgroup_size` (the test does, for the
kernels of the hand-counted files, and scans their launchers for one-dimensional blocks): v0 as the kernel is entered
is the flat work-item id of a one-dimensional launch (every launcher of this project uses dim3(256); the compiler itself uses v0
unmasked as that id), so `v_readfirstlane_b32 s, v0` is below that size.  The range follows s_add / s_lshr / s_and / s_bfe with
constants and decides scalar comparisons: `wave = tid >> 6 < 4` is how the listing of conv3x3_bf16_c64 shows that a wave issues
five or six patch DMA instructions (`k = wave; k < 23; k += 4`) before its `vmcnt(5)`.

Not modelled: LDS contents written by LDS-DMA (an address question), lgkmcnt, timing.
"""
import heapq
import re
import time

SAT = 64  # vmcnt is a 6-bit field: a number of younger entries >= 64 survives every counted wait just like 64 does

_SYM = re.compile(r"^([0-9a-fA-F]+) <(.+)>:\s*$")
_INS = re.compile(r"^\s+([a-z][a-z0-9_]*)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):\s*((?:[0-9A-Fa-f]{8}\s*)+)")
_VREG = re.compile(r"(?<![A-Za-z0-9_])([va])(?:(\d+)|\[(\d+):(\d+)\])(?![A-Za-z0-9_])")
_SREG = re.compile(r"^s(?:(\d+)|\[(\d+):(\d+)\])$")
_VM_PREFIX = ("buffer_", "global_", "scratch_", "flat_", "tbuffer_")
_LOAD_CLASS = {"scratch_": "scratch", "global_": "global", "buffer_": "buffer", "tbuffer_": "buffer"}   # flat_: none (may return out of order)


def _load_class(mnem):
    for prefix, cls in _LOAD_CLASS.items():
        if mnem.startswith(prefix):
            return cls
    return None


_VM_CACHE = re.compile(r"^buffer_(wbl2|inv|wbinvl1|wbinvl1_vol|gl0_inv|gl1_inv)$")

# scalar instructions the checker knows; anything else that starts with s_ is a finding (unknown scalar memory writes included)
_SALU_KNOWN = re.compile(
    r"^s_(mov|cmov|not|wqm|brev|bcnt0|bcnt1|ff0|ff1|flbit|sext|bitset0|bitset1|abs|add|sub|addc|subb|min|max|cselect|and|or|xor|"
    r"andn2|orn2|nand|nor|xnor|lshl|lshr|ashr|bfm|mul|mul_hi|bfe|absdiff|lshl[1-4]_add|pack_ll|pack_lh|pack_hh|movk|cmovk|"
    r"addk|mulk|quadmask|(and|or|xor|andn2|orn2|nand|nor|xnor|andn1|orn1)_saveexec|getpc)_[a-z0-9_]+$|"
    r"^s_(cmp|cmpk)_(eq|lg|gt|ge|lt|le)_[iu](32|64)$|^s_bitcmp[01]_b(32|64)$|"
    r"^s_(load|buffer_load)_dword(x2|x4|x8|x16)?$|^s_(memtime|memrealtime)$|"
    r"^s_(waitcnt|nop|barrier|setprio|sleep|sendmsg|sendmsghalt|setreg_b32|setreg_imm32_b32|getreg_b32|icache_inv|dcache_inv|"
    r"dcache_inv_vol|code_end|ttracedata|incperflevel|decperflevel|set_gpr_idx_on|set_gpr_idx_off|set_gpr_idx_mode|set_gpr_idx_idx)$")
_SALU_NO_DEST = re.compile(r"^s_(cmp_|cmpk_|bitcmp|waitcnt|nop|barrier|setprio|sleep|sendmsg|setreg|icache|dcache|code_end|ttracedata|"
                           r"incperflevel|decperflevel|set_gpr_idx)")
_SALU_KEEPS_SCC = re.compile(r"^s_(mov_|cmov_|cselect_|mul_i32|mul_hi_|movk_|cmovk_|sext_|brev_|bfm_|pack_|getpc_|ff0_|ff1_|flbit_|bitset|"
                             r"load_|buffer_load_|memtime|memrealtime|waitcnt|nop|barrier|setprio|sleep|sendmsg|setreg|getreg|icache|"
                             r"dcache|code_end|ttracedata|incperflevel|decperflevel|set_gpr_idx)")
_BRANCHES = {"s_branch": None, "s_cbranch_scc0": ("scc", False), "s_cbranch_scc1": ("scc", True), "s_cbranch_vccz": ("vcc", False),
             "s_cbranch_vccnz": ("vcc", True), "s_cbranch_execz": ("exec", False), "s_cbranch_execnz": ("exec", True)}
_OTHER_CONTROL = re.compile(r"^s_(setpc|swappc|call|cbranch_g_fork|cbranch_i_fork|cbranch_join|cbranch_cdbg|rfe|rfe_restore|trap|sethalt|"
                            r"endpgm_saved|endpgm_ordered_ps_done|subvector_loop)")
_BOOL2 = {"s_and_b64": "and", "s_or_b64": "or", "s_xor_b64": "xor", "s_andn2_b64": "andn2", "s_orn2_b64": "orn2", "s_nand_b64": "nand",
          "s_nor_b64": "nor", "s_xnor_b64": "xnor"}
_CMP = re.compile(r"^s_(cmp|cmpk)_(eq|lg|gt|ge|lt|le)_([iu])(32|64)$")


class Finding:
    def __init__(self, kind, addr, text, reg=None, count=None, trail=()):
        self.kind, self.addr, self.text, self.reg, self.count, self.trail = kind, addr, text, reg, count, trail

    def __repr__(self):
        s = f"{self.kind} at {self.addr:#x}: {self.text}"
        if self.reg is not None:
            s += f"  [pending {reg_name(self.reg)} with {self.count} younger queue entr{'y' if self.count == 1 else 'ies'}]"
        if self.trail:
            s += "  path: " + " ; ".join(self.trail[-10:])
        return s


def reg_name(r):
    return f"a{r - 1000}" if r >= 1000 else f"v{r}"


class Ins:
    __slots__ = ("addr", "mnem", "ops", "text", "regs", "vm", "dest", "wait", "target", "cond", "kills", "salu", "index", "region", "pad", "wv0")


def _vregs(s):
    out = set()
    for m in _VREG.finditer(s):
        base = 1000 if m.group(1) == "a" else 0
        if m.group(2) is not None:
            out.add(base + int(m.group(2)))
        else:
            out.update(range(base + int(m.group(3)), base + int(m.group(4)) + 1))
    return out


def _sregs(tok):
    """SGPR numbers an operand token names; 'vcc' for vcc and its halves."""
    m = _SREG.match(tok)
    if m:
        return list(range(int(m.group(2)), int(m.group(3)) + 1)) if m.group(1) is None else [int(m.group(1))]
    if tok.startswith("vcc"):
        return ["vcc"]
    return []


def _split_ops(s):
    ops, mods = [], []
    for i, piece in enumerate(p.strip() for p in s.split(",")) if s else []:
        toks = piece.split()
        if not toks:
            continue
        ops.append(toks[0])
        mods += toks[1:]
    return ops, mods


def _decode(mnem, opstr, addr, enc):
    I = Ins()
    I.addr, I.mnem, I.text = addr, mnem, (mnem + " " + opstr).strip()
    ops, mods = _split_ops(opstr)
    if mnem == "s_waitcnt":
        ops, mods = [], opstr.split()
    I.ops = ops
    I.regs = frozenset(_vregs(opstr))
    I.vm = I.dest = I.wait = I.target = I.cond = None
    I.kills, I.salu, I.region = (), False, False
    I.wv0 = bool(ops) and not mnem.startswith("s_") and (0 in _vregs(ops[0]) or (mnem.startswith("v_swap") and 0 in _vregs(opstr)))
    I.pad = not enc.strip("0 \t")      # an all-zero word: padding that the disassembler prints as an instruction
    if mnem.startswith(_VM_PREFIX):
        if _VM_CACHE.match(mnem):
            I.vm = "cache"     # cache control: not counted (counting an entry that does not exist could hide a hazard)
        elif "_load" in mnem:
            lds = "lds" in mods
            I.vm = "lds_dma" if lds else "load"
            if not lds and ops:
                I.dest = frozenset(_vregs(ops[0]))
        elif "_store" in mnem:
            I.vm = "store"
        elif "_atomic" in mnem:
            I.vm = "atomic"
            if ("glc" in mods or "sc0" in mods) and ops:
                I.dest = frozenset(_vregs(ops[0]))
        else:
            I.vm = "unknown"
    elif mnem == "s_waitcnt":
        m = re.search(r"vmcnt\((\d+)\)", opstr)
        if m:
            I.wait = int(m.group(1))
        elif opstr and "cnt(" not in opstr:
            x = int(opstr, 0)
            I.wait = (x & 0xF) | (((x >> 14) & 3) << 4)
            if I.wait == 63:
                I.wait = None
    elif mnem in _BRANCHES:
        simm = int(ops[0], 0) & 0xFFFF
        I.target = addr + 4 + 4 * (simm - 0x10000 if simm & 0x8000 else simm)
        I.cond = _BRANCHES[mnem]
    if mnem.startswith("s_"):
        I.salu = True
        kills = []
        if not _SALU_NO_DEST.match(mnem) and mnem not in _BRANCHES and mnem != "s_endpgm" and ops:
            kills += _sregs(ops[0])
        if "saveexec" in mnem or (ops and ops[0].startswith("exec")):
            kills.append("exec")
        I.kills = tuple(kills)
    elif not I.vm:
        # VALU / LDS / ...: an SGPR or vcc in a destination position (vdst, sdst) is overwritten with something unknown
        kills = []
        for tok in ops[:2]:
            kills += _sregs(tok)
        if mnem.startswith("v_cmpx"):
            kills.append("exec")
        I.kills = tuple(kills)
    return I


class Function:
    def __init__(self, name, addr):
        self.name, self.addr, self.ins = name, addr, []


def parse(listing):
    """objdump text -> list of Function (one per symbol of the text section)."""
    funcs, cur = [], None
    for line in listing.splitlines():
        m = _SYM.match(line)
        if m:
            cur = Function(m.group(2), int(m.group(1), 16))
            funcs.append(cur)
            continue
        m = _INS.match(line)
        if m and cur is not None:
            I = _decode(m.group(1), m.group(2), int(m.group(3), 16), m.group(4))
            I.index = len(cur.ins)
            cur.ins.append(I)
    return funcs


# ---------------------------------------------------------------------------------------------------------------------------
# a small reduced ordered BDD: 0 = false, 1 = true, node n >= 2 = (var, lo, hi)
class Bdd:
    def __init__(self):
        self.nodes = [None, None]
        self.uniq = {}
        self.memo = {}
        self.vars = {}     # atom key -> variable number
        self.keys = []

    def var(self, key):
        v = self.vars.get(key)
        if v is None:
            v = self.vars[key] = len(self.keys)
            self.keys.append(key)
        return self.mk(v, 0, 1)

    def mk(self, v, lo, hi):
        if lo == hi:
            return lo
        k = (v, lo, hi)
        n = self.uniq.get(k)
        if n is None:
            n = self.uniq[k] = len(self.nodes)
            self.nodes.append(k)
        return n

    def neg(self, f):
        if f < 2:
            return 1 - f
        k = ("n", f)
        r = self.memo.get(k)
        if r is None:
            v, lo, hi = self.nodes[f]
            r = self.memo[k] = self.mk(v, self.neg(lo), self.neg(hi))
        return r

    def and_(self, f, g):
        if f == g or g == 1:
            return f
        if f == 1:
            return g
        if f == 0 or g == 0:
            return 0
        if f > g:
            f, g = g, f
        k = ("a", f, g)
        r = self.memo.get(k)
        if r is None:
            vf, vg = self.nodes[f][0], self.nodes[g][0]
            v = min(vf, vg)
            f0, f1 = self.nodes[f][1:] if vf == v else (f, f)
            g0, g1 = self.nodes[g][1:] if vg == v else (g, g)
            r = self.memo[k] = self.mk(v, self.and_(f0, g0), self.and_(f1, g1))
        return r

    def or_(self, f, g):
        return self.neg(self.and_(self.neg(f), self.neg(g)))

    def xor(self, f, g):
        return self.or_(self.and_(f, self.neg(g)), self.and_(self.neg(f), g))

    def support(self, f):
        k = ("s", f)
        r = self.memo.get(k)
        if r is None:
            if f < 2:
                r = frozenset()
            else:
                v, lo, hi = self.nodes[f]
                r = self.support(lo) | self.support(hi) | {v}
            self.memo[k] = r
        return r

    def exists(self, f, v):
        if f < 2:
            return f
        k = ("e", f, v)
        r = self.memo.get(k)
        if r is None:
            fv, lo, hi = self.nodes[f]
            if fv > v:
                r = f
            elif fv == v:
                r = self.or_(lo, hi)
            else:
                r = self.mk(fv, self.exists(lo, v), self.exists(hi, v))
            self.memo[k] = r
        return r

    def describe(self, f):
        """one satisfying assignment of f, in words"""
        out = []
        while f >= 2:
            v, lo, hi = self.nodes[f]
            if hi != 0:
                out.append(_atom_words(self.keys[v], True))
                f = hi
            else:
                out.append(_atom_words(self.keys[v], False))
                f = lo
        return out


def _val_words(v):
    if v[0] == "c":
        return hex(v[1]) if abs(v[1]) > 9 else str(v[1])
    if v[0] == "p":
        return "{" + _val_words(v[1]) + "," + _val_words(v[2]) + "}"
    if v[0] == "tid":
        return "tid"
    if v[0] in ("add", "lshr", "and", "bfe"):
        return f"({_val_words(v[1])} {v[0]} {', '.join(map(str, v[2:]))})"
    return f"<{v[2]} read at {v[1]:#x}>"


def _atom_words(key, truth):
    if key[0] == "cmp":
        return f"{'' if truth else 'not '}{_val_words(key[2])} {key[1]} {_val_words(key[3])}"
    if key[0] == "bit":
        return f"bit {_val_words(key[2])} of {_val_words(key[1])} is {int(truth)}"
    if key[0] == "any":
        return f"{'some' if truth else 'no'} lane in exec {'&' if key[1] == 'and' else '& ~'} {_val_words(key[2])}"
    if key[0] == "exec":
        return f"exec {'non-empty' if truth else 'empty'} at {key[1]:#x}"
    return f"scc read at {key[1]:#x} is {int(truth)}"


# ---------------------------------------------------------------------------------------------------------------------------
class State:
    __slots__ = ("C", "pairs", "vcc", "scc", "sregs", "vbool", "pend", "scr", "trail", "_pk", "_bk")

    def copy(self):
        s = State()
        s.C, s.pairs, s.vcc, s.scc, s.sregs, s.pend, s.trail = self.C, dict(self.pairs), self.vcc, self.scc, dict(self.sregs), dict(self.pend), self.trail
        s.vbool = dict(self.vbool)
        s.scr = self.scr
        s._pk = s._bk = None
        return s

    def bool_key(self):
        if self._bk is None:
            self._bk = self._bool_key()
        return self._bk

    def _bool_key(self):
        return (self.C, frozenset(self.pairs.items()), self.vcc, self.scc, frozenset(self.sregs.items()), frozenset(self.vbool.items()))

    def pend_key(self):
        if self._pk is None:
            self._pk = (frozenset(self.pend.items()), self.scr)
        return self._pk


class Result:
    def __init__(self, name):
        self.name = name
        self.findings = []
        self.tight = {}        # address of a wait -> N, where some register it retires has exactly N younger entries on a feasible path
        self.stats = {}

    @property
    def clean(self):
        return not self.findings


class _Analysis:
    def __init__(self, fn, nonempty_exec, conditions, max_states, max_visits, max_workgroup=None):
        self.fn, self.nonempty_exec, self.conditions = fn, nonempty_exec, conditions
        self.max_workgroup = max_workgroup
        self.max_states, self.max_visits = max_states, max_visits
        self.bdd = Bdd()
        self.res = Result(fn.name)
        self.found = {}
        self.reached = set()
        self.second_pass = False
        self.atoms_of = {}      # value -> the atoms (variable numbers) that mention it

    # ---- findings
    def report(self, kind, I, reg=None, count=None, st=None):
        k = (kind, I.addr, reg)
        old = self.found.get(k)
        if old is None or (count is not None and count < old.count):
            trail = ()
            if st is not None:
                trail = tuple(st.trail) + (("assuming " + ", ".join(self.bdd.describe(st.C))) if st.C >= 2 else "no assumption",)
            self.found[k] = Finding(kind, I.addr, I.text, reg, count, trail)

    # ---- scalar values
    def forget_atoms(self, st, dead):
        """existentially quantify the atoms (variable numbers) `dead` out of the path's assumption; values that depend on them go unknown"""
        b = self.bdd
        for v in sorted(dead, reverse=True):
            st.C = b.exists(st.C, v)
        for r in [r for r, f in st.pairs.items() if b.support(f) & dead]:
            del st.pairs[r]
        if st.vcc is not None and b.support(st.vcc) & dead:
            st.vcc = None
        if st.scc is not None and b.support(st.scc) & dead:
            st.scc = None
        for r in [r for r, (f, _) in st.vbool.items() if b.support(f) & dead]:
            del st.vbool[r]

    def fresh_value(self, st, I, opidx, what):
        """a number for the unknown value read here; an older value numbered at the same place (a previous loop iteration) is forgotten first"""
        vid = ("id", I.addr, what, opidx)
        held = [r for r, v in st.sregs.items() if v == vid or v == ("not", vid)]
        dead = self.atoms_of.get(vid)
        dead = (dead & self.live_atoms(st)) if dead else None
        for r in held:
            del st.sregs[r]
        if dead:
            self.forget_atoms(st, dead)
        return vid

    def live_atoms(self, st):
        b = self.bdd
        s = set(b.support(st.C))
        for f in st.pairs.values():
            s |= b.support(f)
        for f in (st.vcc, st.scc):
            if f is not None:
                s |= b.support(f)
        for f, _ in st.vbool.values():
            s |= b.support(f)
        return s

    def range_of(self, v):
        """(lo, hi) of a value built from the work-item id by constants, or None.  ("tid",) is v0 as the kernel was entered, read by
        v_readfirstlane_b32: below the code object's .max_flat_workgroup_size (see the module docstring)."""
        k = v[0]
        if k == "c":
            return (v[1], v[1])
        if k == "tid":
            return (0, self.max_workgroup - 1)
        if k in ("add", "lshr", "and", "bfe"):
            r = self.range_of(v[1])
            if r is None:
                return None
            lo, hi = r
            if k == "add":
                return (lo + v[2], hi + v[2])
            if lo < 0:
                return None
            if k == "lshr":
                return (lo >> v[2], hi >> v[2])
            if k == "and":
                return (0, min(hi, v[2])) if v[2] >= 0 else None
            return (0, min(hi >> v[2], (1 << v[3]) - 1))
        return None

    def term(self, st, I):
        """s_add / s_lshr / s_and / s_bfe of a ranged value and a constant -> the value of the result, or None.  Only values that
        come from the work-item id are followed, and only a little way: that keeps loops finite."""
        m = re.match(r"^s_(add_[iu]32|lshr_b32|and_b32|bfe_u32)$", I.mnem)
        if not m or len(I.ops) != 3:
            return None
        op = m.group(1).split("_")[0]
        a, c = I.ops[1], I.ops[2]
        if op in ("add", "and") and not _SREG.match(a):
            a, c = c, a
        ma = _SREG.match(a)
        if not ma or ma.group(1) is None:
            return None
        v = st.sregs.get(int(ma.group(1)))
        try:
            k = int(c, 0)
        except ValueError:
            return None
        if v is None or v[0] == "c" or self.range_of(v) is None:
            return None
        if op == "add":
            if v[0] == "add":
                v, k = v[1], v[2] + k
            t = ("add", v, k) if k else v
        elif op == "bfe":
            t = ("bfe", v, k & 31, (k >> 16) & 127)
        else:
            t = (op, v, k)
        r = self.range_of(t)
        return t if r is not None and -64 <= r[0] and r[1] <= 4096 and (t[0] != "add" or abs(t[2]) <= 64) else None

    def sval(self, st, I, opidx, tok):
        """value of a 32-bit scalar operand"""
        if _SREG.match(tok):
            r = _sregs(tok)[0]
            v = st.sregs.get(r)
            if v is None:
                v = st.sregs[r] = self.fresh_value(st, I, opidx, tok)
            return v
        try:
            return ("c", int(tok, 0))
        except ValueError:
            return self.fresh_value(st, I, opidx, tok)   # m0, exec_lo, literal floats, ...: unknown, never equal to anything older

    def pair_bool(self, st, tok):
        """boolean function of a 64-bit operand, or None when nothing is known about it"""
        if tok == "-1":
            return 1
        if tok == "0":
            return 0
        if tok == "vcc":
            return st.vcc
        m = _SREG.match(tok)
        if m and m.group(1) is None and int(m.group(3)) == int(m.group(2)) + 1:
            return st.pairs.get(int(m.group(2)))
        return None

    def set_pair(self, st, tok, f):
        if tok == "vcc":
            st.vcc = f
            return
        m = _SREG.match(tok)
        if m and m.group(1) is None and f is not None:
            st.pairs[int(m.group(2))] = f

    def kill(self, st, I):
        for r in I.kills:
            if r == "vcc":
                st.vcc = None
            elif r == "exec":
                self.new_exec(st, ("x", I.addr))
            else:
                st.sregs.pop(r, None)
                st.pairs.pop(r & ~1, None)
                st.sregs.pop(("saved", r & ~1), None)
                st.sregs.pop(("mask", r & ~1), None)

    def new_exec(self, st, ev):
        """exec holds a new value, named by where it was written; what a VGPR was said to hold under an older value of that name goes"""
        st.sregs["exec"] = ev
        for r in [r for r, (_, e) in st.vbool.items() if e == ev]:
            del st.vbool[r]

    def vector(self, st, I):
        """a uniform condition that travels through a VGPR: v_cndmask_b32 v, 0, 1, pair ... v_cmp_ne_u32 pair', 1, v.  Valid while exec
        is the value it was when the VGPR was written (every lane the compare reads was written by the select)."""
        ops, mnem = I.ops, I.mnem
        if st.vbool and ops:
            for r in _vregs(ops[0]) | (_vregs(ops[1]) if mnem.startswith("v_swap") and len(ops) > 1 else set()):
                st.vbool.pop(r, None)
        if mnem == "v_cndmask_b32_e64" and len(ops) == 4 and (ops[1], ops[2]) in (("0", "1"), ("1", "0")):
            f, ev, d = self.pair_bool(st, ops[3]), st.sregs.get("exec", ("x", 0)), _vregs(ops[0])
            if f is not None and len(d) == 1:
                st.vbool[d.pop()] = (f if ops[1] == "0" else self.bdd.neg(f), ev)
            return None
        m = re.match(r"^v_cmp_(eq|ne)_[iu]32_e(32|64)$", mnem)
        if m and len(ops) == 3:
            k, v = (ops[1], ops[2]) if ops[1] in ("0", "1") else (ops[2], ops[1])
            rv = _vregs(v)
            if k in ("0", "1") and len(rv) == 1:
                got = st.vbool.get(next(iter(rv)))
                if got is not None and got[1] == st.sregs.get("exec", ("x", 0)):
                    return got[0] if (m.group(1) == "eq") == (k == "1") else self.bdd.neg(got[0])
        return None

    def atom(self, st, key):
        if key not in self.bdd.vars:
            f = self.bdd.var(key)
            for leaf in _leaves(key):
                self.atoms_of.setdefault(leaf, set()).add(self.bdd.vars[key])
            return f
        return self.bdd.var(key)

    def scalar(self, st, I):
        """effect of a scalar instruction on the tracked conditions"""
        b, mnem, ops = self.bdd, I.mnem, I.ops
        m = _CMP.match(mnem)
        if m:
            _, rel, sign, width = m.groups()
            f = None
            if width == "64":
                pb = self.pair_bool(st, ops[0]) if ops[1] == "0" else None
                if pb is not None and rel in ("eq", "lg"):
                    f = pb if rel == "lg" else b.neg(pb)
                else:
                    va = self.val64(st, I, 0, ops[0])
                    vb = self.val64(st, I, 1, ops[1])
            else:
                va, vb = self.sval(st, I, 0, ops[0]), self.sval(st, I, 1, ops[1])
            if f is None:
                f = self.compare(st, rel, sign + width, va, vb)
            st.scc = f
            return
        if mnem.startswith("s_bitcmp"):
            va = self.val64(st, I, 0, ops[0]) if mnem.endswith("64") else self.sval(st, I, 0, ops[0])
            f = self.atom(st, ("bit", va, self.sval(st, I, 1, ops[1])))
            st.scc = f if mnem.startswith("s_bitcmp1") else b.neg(f)
            return
        t = self.term(st, I) if self.max_workgroup else None
        if t is not None:
            self.kill(st, I)
            d = _sregs(ops[0])
            if d and d[0] != "vcc":
                st.sregs[d[0]] = t
            st.scc = None
            return
        if mnem == "s_mov_b32":
            v = self.sval(st, I, 1, ops[1])
            self.kill(st, I)
            d = _sregs(ops[0])
            if d and d[0] != "vcc":
                st.sregs[d[0]] = v
            return
        if mnem == "s_mov_b64":
            f = self.pair_bool(st, ops[1])
            halves = None
            m2 = _SREG.match(ops[1])
            if m2 and m2.group(1) is None:
                lo = int(m2.group(2))
                halves = (st.sregs.get(lo), st.sregs.get(lo + 1))
            elif ops[1] in ("0", "-1"):
                halves = (("c", int(ops[1])), ("c", int(ops[1])))
            mv = st.sregs.get(("mask", int(m2.group(2)))) if m2 and m2.group(1) is None else None
            self.kill(st, I)
            self.set_pair(st, ops[0], f)
            d = _sregs(ops[0])
            if mv is not None and len(d) == 2:
                st.sregs[("mask", d[0])] = mv
            if halves and len(d) == 2:
                for r, v in zip(d, halves):
                    if v is not None:
                        st.sregs[r] = v
            return
        if mnem == "s_cselect_b64" and ops[1] in ("0", "-1") and ops[2] in ("0", "-1"):
            if st.scc is None:
                dead = {n for k, n in b.vars.items() if k == ("scc", I.addr)} & self.live_atoms(st)
                if dead:
                    self.forget_atoms(st, dead)
                st.scc = self.atom(st, ("scc", I.addr))
            t, e = self.pair_bool(st, ops[1]), self.pair_bool(st, ops[2])
            f = b.or_(b.and_(st.scc, t), b.and_(b.neg(st.scc), e))
            self.kill(st, I)
            self.set_pair(st, ops[0], f)
            return
        if mnem in _BOOL2 or mnem == "s_not_b64":
            f = None
            if ops[0].startswith("exec"):
                # leaving a divergent region: `s_or_b64 exec, exec, saved` gives exec the value it had at the saveexec
                m2 = _SREG.match(ops[2]) if mnem == "s_or_b64" and len(ops) == 3 and ops[1] == "exec" else None
                ev = st.sregs.get(("saved", int(m2.group(2)))) if m2 and m2.group(1) is None else None
                self.kill(st, I)
                if ev is not None:
                    st.sregs["exec"] = ev
                st.scc = None
                return
            elif mnem == "s_not_b64":
                a = self.pair_bool(st, ops[1])
                f = None if a is None else b.neg(a)
            elif ops[1] == "exec" or ops[2] == "exec":
                # vcc = exec & pair / exec & ~pair: "some lane of a uniform condition"
                other = ops[2] if ops[1] == "exec" else ops[1]
                a = self.pair_bool(st, other)
                op = _BOOL2[mnem]
                if a is None and (op == "and" or (op == "andn2" and ops[1] == "exec")):
                    f = self.mask_test(st, I, other, op)
                elif a is not None and (op == "and" or (op == "andn2" and ops[1] == "exec")):
                    f = a if op == "and" else b.neg(a)
                    if not self.nonempty_exec:
                        dead = {n for k, n in b.vars.items() if k == ("exec", I.addr)} & self.live_atoms(st)
                        if dead:
                            self.forget_atoms(st, dead)
                        f = b.and_(f, self.atom(st, ("exec", I.addr)))
            else:
                a, c = self.pair_bool(st, ops[1]), self.pair_bool(st, ops[2])
                op = _BOOL2[mnem]
                # a known false / true operand decides and / or whatever the other operand is
                if op == "and" and (a == 0 or c == 0):
                    f = 0
                elif op == "andn2" and (a == 0 or c == 1):
                    f = 0
                elif op == "or" and (a == 1 or c == 1):
                    f = 1
                elif a is not None and c is not None:
                    nc = b.neg(c)
                    f = {"and": lambda: b.and_(a, c), "or": lambda: b.or_(a, c), "xor": lambda: b.xor(a, c),
                         "andn2": lambda: b.and_(a, nc), "orn2": lambda: b.or_(a, nc),
                         "nand": lambda: b.neg(b.and_(a, c)), "nor": lambda: b.neg(b.or_(a, c)),
                         "xnor": lambda: b.neg(b.xor(a, c))}[op]()
            comp = None
            if f is None and not ops[0].startswith(("exec", "vcc")):
                src = ops[1] if mnem == "s_not_b64" or (mnem == "s_xor_b64" and ops[2] == "-1") else ops[2] if (mnem == "s_xor_b64" and ops[1] == "-1") else None
                m2 = _SREG.match(src) if src else None
                if m2 and m2.group(1) is None and self.pair_bool(st, src) is None:
                    mv = self.mask_value(st, I, int(m2.group(2)), src)
                    comp = mv[1] if mv[0] == "not" else ("not", mv)
            self.kill(st, I)
            self.set_pair(st, ops[0], f)
            d = _sregs(ops[0])
            if comp is not None and len(d) == 2:
                st.sregs[("mask", d[0])] = comp
            st.scc = None    # (SCC = result is non-zero, but a pair that came through a v_cmp is zero outside exec: leave it unknown)
            return
        if "saveexec" in mnem:
            ev = st.sregs.get("exec")
            self.kill(st, I)
            d = _sregs(ops[0])
            if ev is not None and len(d) == 2:
                st.sregs[("saved", d[0])] = ev
            st.scc = None
            return
        self.kill(st, I)
        if not _SALU_KEEPS_SCC.match(mnem):
            st.scc = None

    def mask_test(self, st, I, tok, op):
        """`exec & mask` / `exec & ~mask` of a pair the checker knows nothing about (a lane mask): whether any lane is left is one
        unknown truth per (value of the mask, value of exec, operation) - the same test of the same values gives the same answer"""
        m = _SREG.match(tok)
        ev = st.sregs.get("exec", ("x", 0))
        if not m or m.group(1) is not None or ev is None:
            return None
        mv = self.mask_value(st, I, int(m.group(2)), tok)
        if mv[0] == "not":     # exec & ~~m = exec & m
            mv, op = mv[1], ("andn2" if op == "and" else "and")
        return self.atom(st, ("any", op, mv, ev))

    def mask_value(self, st, I, lo, tok):
        mv = st.sregs.get(("mask", lo))
        if mv is None:
            mv = st.sregs[("mask", lo)] = self.fresh_value(st, I, 0, tok)
        return mv

    def val64(self, st, I, opidx, tok):
        m = _SREG.match(tok)
        if m and m.group(1) is None:
            lo = int(m.group(2))
            return ("p", self.sval(st, I, 2 * opidx, f"s{lo}"), self.sval(st, I, 2 * opidx + 1, f"s{lo + 1}"))
        return self.sval(st, I, opidx, tok)

    def compare(self, st, rel, ty, va, vb):
        b = self.bdd
        ra, rb = self.range_of(va), self.range_of(vb)
        if ra is not None and rb is not None and ty.endswith("32") and (ty[0] == "i" or (ra[0] >= 0 and rb[0] >= 0)) \
                and not (va[0] == "c" and vb[0] == "c"):
            # the ranges decide the comparison (values that come from the work-item id)
            lt = 1 if ra[1] < rb[0] else 0 if ra[0] >= rb[1] else None
            gt = 1 if ra[0] > rb[1] else 0 if ra[1] <= rb[0] else None
            eq = 0 if (ra[1] < rb[0] or ra[0] > rb[1]) else 1 if ra == rb and ra[0] == ra[1] else None
            d = {"lt": lt, "gt": gt, "eq": eq, "ge": None if lt is None else 1 - lt, "le": None if gt is None else 1 - gt,
                 "lg": None if eq is None else 1 - eq}[rel]
            if d is not None:
                return d
        if va[0] == "c" and vb[0] == "c" and rel in ("eq", "lg"):
            mask = (1 << int(ty[1:])) - 1
            eq = (va[1] & mask) == (vb[1] & mask)
            return 1 if eq == (rel == "eq") else 0
        neg = False
        if rel == "lg":
            rel, neg = "eq", True
        elif rel == "ge":
            rel, neg = "lt", True
        elif rel == "le":
            rel, neg = "gt", True
        if rel == "gt":
            rel, va, vb = "lt", vb, va
        if rel == "eq":
            if va == vb:
                return 0 if neg else 1
            if repr(va) > repr(vb):
                va, vb = vb, va
            ty = ty[1:]
        elif va == vb:
            return 1 if neg else 0
        f = self.atom(st, ("cmp", rel + "_" + ty, va, vb))
        return b.neg(f) if neg else f

    # ---- one state through one block
    def constrain(self, st, f):
        """narrow the path's assumption.  Values stay as they are: a value rewritten to what it is worth under the assumption
        would be wrong once the assumption is forgotten."""
        st.C = self.bdd.and_(st.C, f)

    def gc(self, st):
        """forget assumptions about values that nothing can test again"""
        b = self.bdd
        need = set()
        for f in st.pairs.values():
            need |= b.support(f)
        for f in (st.vcc, st.scc):
            if f is not None:
                need |= b.support(f)
        for f, _ in st.vbool.values():
            need |= b.support(f)
        sup = b.support(st.C)
        if sup <= need:
            return
        held = set(st.sregs.values())
        held |= {v[1] for v in held if v[0] == "not"}
        dead = set()
        for v in sup - need:
            k = b.keys[v]
            if k[0] in ("cmp", "bit", "any") and all(x in held or x[0] in ("c", "x", "tid") for x in _leaves(k)):
                continue    # the same values can be compared again
            dead.add(v)
        if dead:
            self.forget_atoms(st, dead)

    def run_block(self, blk, st):
        """-> list of (successor address, state)"""
        ins = self.fn.ins
        b = self.bdd
        i, end = blk
        while True:
            I = ins[i]
            self.reached.add(i)
            if I.wv0:
                st.sregs.pop("v0", None)
            pend = st.pend
            if pend and I.regs and not I.regs.isdisjoint(pend):
                hit = I.regs & pend.keys()
                if I.dest and I.vm == "load" and hit <= I.dest and hit.isdisjoint(_vregs(" ".join(I.ops[1:]))) \
                        and _load_class(I.mnem) is not None and all((r, _load_class(I.mnem)) in st.scr for r in hit):
                    hit = ()     # a load over a pending load of the same class (scratch / global / buffer): they return in order, the
                                 # younger value wins, and the compiler emits this itself (a reload hoisted above a branch)
                for r in sorted(hit):
                    self.report("hazard", I, r, pend[r], st)
            if I.vm:
                if I.vm == "unknown":
                    self.report("unknown vector-memory instruction", I)
                elif I.vm != "cache":
                    if pend:
                        st.pend = pend = {r: (n + 1 if n < SAT else n) for r, n in pend.items()}
                    if I.dest:
                        if not pend:
                            st.pend = pend = {}
                        for r in I.dest:
                            pend[r] = 0
                            if st.vbool:
                                st.vbool.pop(r, None)
                        st.scr = frozenset(x for x in st.scr if x[0] not in I.dest) | {(r, _load_class(I.mnem)) for r in I.dest}
            elif I.wait is not None:
                if pend:
                    n = I.wait
                    if any(c == n for c in pend.values()):
                        self.res.tight[I.addr] = n
                    st.pend = {r: c for r, c in pend.items() if c < n}
                    if st.scr:
                        st.scr = frozenset(x for x in st.scr if x[0] in st.pend)
            elif I.salu:
                if I.mnem == "s_endpgm":
                    return []
                if I.mnem in _BRANCHES:
                    return self.branch(st, I, ins[i + 1].addr if i + 1 < len(ins) else None)
                if _OTHER_CONTROL.match(I.mnem):
                    self.report("unknown control flow", I)
                    return []
                if not _SALU_KNOWN.match(I.mnem):
                    self.report("unknown scalar instruction", I)
                if self.conditions:
                    self.scalar(st, I)
            else:
                if not (I.mnem.startswith("v_") or I.mnem.startswith("ds_")):
                    self.report("unknown instruction class", I)
                if self.conditions:
                    f = self.vector(st, I) if (st.vbool or I.mnem.startswith(("v_cndmask", "v_cmp_"))) else None
                    if I.kills:
                        self.kill(st, I)
                    if I.mnem == "v_readfirstlane_b32" and I.ops[1] == "v0" and "v0" in st.sregs and _SREG.match(I.ops[0]):
                        st.sregs[_sregs(I.ops[0])[0]] = ("tid",)
                    if f is not None:
                        self.set_pair(st, I.ops[0], f)
            if i == end:
                if i + 1 >= len(ins):
                    self.report("control runs off the end of the function", I)
                    return []
                return [(ins[i + 1].addr, st)]
            i += 1

    def branch(self, st, I, fall):
        b = self.bdd
        if I.cond is None:
            return [(I.target, st)]
        which, sense = I.cond
        out = []
        if which == "exec":
            if self.nonempty_exec and I.region:
                return [(I.target, st)] if sense else ([(fall, st)] if fall is not None else [])
            f = None    # any other branch on exec (the back edge or exit of a divergent loop, which ends when no lane is left): both ways
        else:
            f = (st.scc if which == "scc" else st.vcc) if self.conditions else None
        for taken in (True, False):
            dst = I.target if taken else fall
            if dst is None:
                self.report("control runs off the end of the function", I)
                continue
            s2 = st.copy()
            if f is not None:
                g = b.and_(st.C, f if taken == sense else b.neg(f))
                if g == 0:
                    continue
                if g != st.C:
                    self.constrain(s2, g)
                    s2.trail = st.trail + (f"{I.addr:#x} {I.mnem} {'taken' if taken else 'not taken'}",)
            out.append((dst, s2))
        return out

    # ---- states at block entries
    def merge_into(self, lst, st):
        """merge `st` into the states `lst` of a block entry; -> the state to (re)run, or None when nothing new arrived"""
        b = self.bdd
        pk = st.pend_key()
        for old in lst:
            if old.pend_key() == pk and self.same_knowledge(old, st) and self.agree(old, st):
                return self.merge_bool(old, st)
        bk = st.bool_key()
        for old in lst:
            if old.bool_key() == bk:
                return self.merge_pend(old, st)
        if len(lst) >= self.max_states:
            old = lst[0]
            ch1 = self.merge_pend(old, st)
            ch2 = self.merge_bool(old, st)
            return old if (ch1 or ch2) else None
        lst.append(st)
        return st

    def agree(self, a, c):
        """where the assumptions of two states overlap, every condition has the same truth in both"""
        b = self.bdd
        both = b.and_(a.C, c.C)
        if both == 0:
            return True
        for r, f in a.pairs.items():
            if b.and_(both, b.xor(f, c.pairs[r])) != 0:
                return False
        for f, g in ((a.vcc, c.vcc), (a.scc, c.scc)):
            if f is not None and b.and_(both, b.xor(f, g)) != 0:
                return False
        return True

    @staticmethod
    def same_knowledge(a, b):
        """two states are folded into one only when that forgets no condition: both know the same pairs and condition codes
        and agree on exec, saved exec masks and the identities of lane masks"""
        if a.pairs.keys() != b.pairs.keys() or (a.vcc is None) != (b.vcc is None) or (a.scc is None) != (b.scc is None):
            return False
        if a.vbool != b.vbool:
            return False
        ka = {k: v for k, v in a.sregs.items() if not isinstance(k, int)}
        kb = {k: v for k, v in b.sregs.items() if not isinstance(k, int)}
        return ka == kb

    @staticmethod
    def merge_pend(old, st):
        ch = False
        scr = (old.scr & st.scr) | frozenset(x for x in old.scr if x[0] not in st.pend) | frozenset(x for x in st.scr if x[0] not in old.pend)
        for r, n in st.pend.items():
            o = old.pend.get(r)
            if o is None or n < o:
                old.pend[r] = n
                ch = True
        if scr != old.scr:
            old.scr, ch = scr, True
        if ch:
            old._pk = None
        return old if ch else None

    def merge_bool(self, old, st):
        """old := the union of both path sets: assumption C_old | C_new, every value `C_old ? f_old : f_new` (exact where the
        two agree on the overlap of the assumptions, unknown otherwise); -> old when it changed"""
        b = self.bdd
        if old.bool_key() == st.bool_key():
            return None
        newC = b.or_(old.C, st.C)
        both = b.and_(old.C, st.C)
        changed = [newC != old.C]

        def ite(fo, fs):
            if fo is None:
                return None
            if fs is None or (both != 0 and b.and_(both, b.xor(fo, fs)) != 0):
                changed[0] = True
                return None
            if fo == fs:
                return fo
            f = b.or_(b.and_(old.C, fo), b.and_(b.neg(old.C), fs))
            if b.and_(newC, b.xor(f, fo)) == 0:
                return fo
            changed[0] = True
            return f
        pairs = {}
        for r, fo in old.pairs.items():
            f = ite(fo, st.pairs.get(r))
            if f is not None:
                pairs[r] = f
        old.vcc, old.scc = ite(old.vcc, st.vcc), ite(old.scc, st.scc)
        old.pairs = pairs
        sregs = {r: v for r, v in old.sregs.items() if st.sregs.get(r) == v}
        vbool = {r: v for r, v in old.vbool.items() if st.vbool.get(r) == v}
        if len(sregs) != len(old.sregs) or len(vbool) != len(old.vbool):
            changed[0] = True
        old.sregs, old.vbool = sregs, vbool
        old.C = newC
        old._bk = None
        return old if changed[0] else None

    def run(self):
        fn, ins = self.fn, self.fn.ins
        t0 = time.perf_counter()
        res = self.res
        if not ins:
            return res
        # trailing padding after the last terminator is not code
        last = len(ins) - 1
        while last > 0 and (ins[last].mnem in ("s_nop", "s_code_end") or ins[last].pad):
            last -= 1
        if last < len(ins) - 1 and (ins[last].mnem in ("s_endpgm", "s_branch") or _OTHER_CONTROL.match(ins[last].mnem)):
            ins = fn.ins = ins[:last + 1]
        by_addr = {I.addr: I.index for I in ins}
        # a branch on exec is the guard of an if-region when the last write of exec before it is an s_*_saveexec_b64
        for I in ins:
            if I.cond is not None and I.cond[0] == "exec":
                k = I.index - 1
                while k >= 0 and "exec" not in ins[k].kills and ins[k].mnem not in _BRANCHES and ins[k].mnem != "s_endpgm":
                    k -= 1
                I.region = k >= 0 and "saveexec" in ins[k].mnem
        leaders = {0}
        for I in ins:
            if I.mnem in _BRANCHES or I.mnem == "s_endpgm" or _OTHER_CONTROL.match(I.mnem):
                if I.index + 1 < len(ins):
                    leaders.add(I.index + 1)
                if I.target is not None:
                    t = by_addr.get(I.target)
                    if t is None:
                        self.report("branch leaves the function", I)
                    else:
                        leaders.add(t)
        order = sorted(leaders)
        blocks = {s: (s, (order[k + 1] - 1) if k + 1 < len(order) else len(ins) - 1) for k, s in enumerate(order)}
        entry = {s: [] for s in order}
        st = State()
        st.C, st.pairs, st.vcc, st.scc, st.sregs, st.pend, st.trail = 1, {}, None, None, {}, {}, ()
        st.vbool = {}
        st._pk = st._bk = None
        if self.max_workgroup:
            st.sregs["v0"] = ("tid",)      # v0 still holds what the kernel was entered with
        st.scr = frozenset()     # (register, class of its load: _LOAD_CLASS) of every pending register
        entry[0].append(st)
        heap, queued, seq = [(0, 0, st)], {id(st)}, 1
        visits = peak = 0
        while heap:
            s, _, st = heapq.heappop(heap)
            queued.discard(id(st))
            visits += 1
            if visits > self.max_visits:
                self.report("analysis did not converge", ins[s])
                break
            for dst, out in self.run_block(blocks[s], st.copy()):
                t = by_addr.get(dst)
                if t is None:
                    continue     # reported above
                if self.conditions:
                    self.gc(out)
                again = self.merge_into(entry[t], out)
                if again is not None and id(again) not in queued:
                    queued.add(id(again))
                    heapq.heappush(heap, (t, seq, again))
                    seq += 1
                peak = max(peak, len(entry[t]))
        skipped = [I for I in ins if I.index not in self.reached]
        only_without = 0
        if skipped and self.nonempty_exec and not self.second_pass:
            # what the exec assumption cuts off (the path on which a wave skips a guarded region) must still be code the checker
            # can read: walk the function once more with every branch both ways, for reachability and instruction classes only
            other = _Analysis(Function(fn.name, fn.addr), False, False, self.max_states, self.max_visits)
            other.fn.ins, other.second_pass = ins, True
            other.run()
            for k, f in other.found.items():
                if f.kind != "hazard":
                    self.found.setdefault(k, f)
            only_without = sum(1 for I in skipped if I.index in other.reached)
            skipped = [I for I in skipped if I.index not in other.reached]
        for I in skipped:
            self.report("unreachable instruction", I)
        res.findings = sorted(self.found.values(), key=lambda f: (f.addr, f.kind, f.reg or 0))
        q = {}
        for I in ins:
            if I.vm and I.vm != "cache":
                q[I.vm] = q.get(I.vm, 0) + 1
        res.stats = {
            "instructions": len(ins),
            "queue": q,
            "waits_zero": sum(1 for I in ins if I.wait == 0),
            "waits_counted": sum(1 for I in ins if I.wait),
            "tight": len(res.tight),
            "tight_counted": sum(1 for n in res.tight.values() if n),
            "skipped_by_exec_assumption": only_without,
            "peak_states": peak,
            "visits": visits,
            "seconds": time.perf_counter() - t0,
        }
        return res


def _leaves(key):
    out = []
    for x in key[1:]:
        if isinstance(x, tuple):
            if x[0] == "p":
                out += [x[1], x[2]]
            else:
                out.append(x)
    return out


def analyse_function(fn, nonempty_exec=True, conditions=True, max_states=16, max_visits=400000, max_workgroup=None):
    return _Analysis(fn, nonempty_exec, conditions, max_states, max_visits, max_workgroup).run()


def analyse(listing, nonempty_exec=True, conditions=True, only=None, **kw):
    """objdump text -> {symbol: Result}; `only`: a predicate on symbol names"""
    return {fn.name: analyse_function(fn, nonempty_exec, conditions, **kw) for fn in parse(listing) if only is None or only(fn.name)}


def split_functions(listing):
    """{symbol: the lines of that symbol, header included} of a listing"""
    out, cur = {}, None
    for line in listing.splitlines():
        m = _SYM.match(line)
        if m:
            cur = out.setdefault(m.group(2), [])
        if cur is not None and line.strip():
            cur.append(line)
    return out
