"""Wait-state audit of the compiled kernels (no GPU needed):
    python tools/isa_hazards.py [--out profiles/isa_hazards.txt] [file.s ...]
The compiler treats an `asm` statement as ONE opaque instruction: it pads no hazard whose producer or consumer is
inside the string.  This tool compiles every translation unit of csrc/build.sh to assembly with build.sh's own flags
(so the audited code is the shipped code), rebuilds the control flow of every kernel from its labels and branches,
and checks the distance, in wait states, between the instruction pairs that need one — along EVERY static successor
edge (fall-through and branch targets), not along the text.  Assembly is used instead of an object dump because the
`;;#ASMSTART` / `;;#ASMEND` markers tell inline assembly from compiler code.

Wait states are counted the way the compiler's own hazard recogniser counts them: every issued instruction between
producer and consumer is one state, `s_nop N` is N + 1.

Rules (a finding = file, kernel, rule, producer, consumer, states found, states required):
  H1  MFMA result: after an MFMA writes D, no instruction reads or writes a register overlapping D within the required
      states — except an MFMA that takes D WHOLE as its C operand and reads none of it as A or B (accumulate chain).
      The required states are MEASURED: the smallest distance the compiler leaves behind its own (builtin) MFMAs of
      the same shape anywhere in the library (h1_table).
  H2  VALU write -> DPP read of the same VGPR.
  H3  VALU-written SGPR (v_readfirstlane, v_readlane, v_cmp ...) -> global_* / buffer_* reading it.
  H4  LDS-DMA and M0: every global_load_lds_* sits in an asm block behind that block's own `s_mov_b32 m0` and at least
      one state; a kernel with such a DMA mentions m0 nowhere else.
  H5  VALU write -> A / B operand of an INLINE MFMA.
  allow-list: the opcodes that appear in inline assembly anywhere are exactly INLINE_ALLOWED.
Measurement infrastructure."""
import collections
import concurrent.futures
import os
import re
import shlex
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conditional-flow-matching_amd", "csrc")
MAX_JOBS = 16

# Required states.  H1 is measured (h1_table); the others are the software-inserted wait states of the CDNA ISA guides
# ("Manually Inserted Wait States"), which the compiler pads for its own instructions and nobody pads inside asm:
H2_STATES = 2   # VALU writes a VGPR -> a DPP instruction reads it: 2 (`s_nop 1`, as csrc/assign_small.h pads by hand)
H3_STATES = 5   # VALU writes an SGPR -> a VMEM instruction reads it (base, offset, descriptor): 5 (`s_nop 4`)
H5_STATES = 2   # VALU (or v_accvgpr_write) writes a VGPR -> an MFMA reads it as A / B: 2 (`s_nop 1`)
H4_STATES = 1   # s_mov_b32 m0 -> the LDS-DMA that reads it: 1 (`s_nop 0`, as csrc/gemm_glds.h pads by hand)
H1_EXPECTED = {"16x16x4_f32": 10, "32x32x2_f32": 18}      # what the compiler leaves here: passes + 2
RULE_LOOKAHEAD = 6                                         # H2 / H3 / H5: states beyond the requirement searched for the nearest pair
H1_LOOKAHEAD = 40                                          # states to follow behind an MFMA (> any requirement)

# opcode -> predicate on the instruction: everything inline assembly may contain today.  A new inline instruction
# fails tests/test_isa_hazards.py until it is added here TOGETHER with the rule that covers it.
INLINE_ALLOWED = {
    "s_waitcnt": lambda i: True,
    "s_barrier": lambda i: True,
    "s_nop": lambda i: True,
    "s_mov_b32": lambda i: i.ops[:1] == ["m0"],                              # H4
    "global_load_lds_dwordx4": lambda i: True,                               # H4, H3
    "v_mfma_f32_16x16x4_f32": lambda i: True,                                # H1, H5
    "v_min_u32_dpp": lambda i: True,                                         # H2
    "v_med3_u32": lambda i: True,                                            # a plain VALU: a producer of H2 / H5 like any other
    "ds_or_b32": lambda i: True, "ds_and_b32": lambda i: True, "ds_sub_u32": lambda i: True,
    "ds_min_u32": lambda i: True, "ds_max_i32": lambda i: True,              # LDS atomics without a result: no register written
}

Finding = collections.namedtuple("Finding", "file kernel rule producer consumer found required")

_REG_RANGE = re.compile(r"\b([vas])\[(\d+):(\d+)\]")
_REG_ONE = re.compile(r"\b([vas])(\d+)\b")
_SPECIAL = re.compile(r"\b(vcc|exec|m0|scc)(?:_lo|_hi)?\b")
_DPP = re.compile(r"\b(quad_perm|row_shl|row_shr|row_ror|wave_shl|wave_shr|wave_rol|wave_ror|row_mirror|row_half_mirror|"
                  r"row_bcast|row_share|row_xmask|row_newbcast|dpp8)\b")
_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_TWO_DEST = ("v_add_co_", "v_sub_co_", "v_subrev_co_", "v_addc_co_", "v_subb_co_", "v_subbrev_co_", "v_div_scale_",
             "v_mad_u64_u32", "v_mad_i64_i32", "v_swap_")


def regs_of(text):
    """the registers a piece of operand text names: {("v", 3), ("s", 10), ("vcc", 0), ...}"""
    out = set()
    for f, a, b in _REG_RANGE.findall(text):
        out.update((f, n) for n in range(int(a), int(b) + 1))
    for f, a in _REG_ONE.findall(text):
        out.add((f, int(a)))
    for s in _SPECIAL.findall(text):
        out.add((s, 0))
    return out


def _split_ops(text):
    ops, depth, cur = [], 0, ""
    for ch in text:
        if ch == "[":
            depth += 1
        elif ch == "]":
            depth -= 1
        if ch == "," and depth == 0:
            ops.append(cur.strip()); cur = ""
        else:
            cur += ch
    if cur.strip():
        ops.append(cur.strip())
    return ops


class Instr:
    __slots__ = ("line", "text", "op", "ops", "inline", "block", "opregs", "regs", "succ", "states", "is_mfma",
                 "is_valu", "is_dpp", "writes")

    def __init__(self, line, text, inline, block):
        self.line, self.text, self.inline, self.block = line, text, inline, block
        parts = text.split(None, 1)
        self.op = parts[0]
        self.ops = _split_ops(parts[1]) if len(parts) > 1 else []
        self.opregs = [regs_of(o) for o in self.ops]
        self.regs = set().union(*self.opregs) if self.opregs else set()
        self.succ = []
        self.states = 1
        if self.op == "s_nop":
            self.states = int(self.ops[0], 0) + 1
        self.is_mfma = self.op.startswith("v_mfma") or self.op.startswith("v_smfmac")
        self.is_valu = self.op.startswith("v_") and not self.is_mfma
        self.is_dpp = self.op.endswith("_dpp") or bool(_DPP.search(text))
        # registers written: the first operand (the first two where the opcode has a second destination); a VALU compare
        # prints its SGPR / vcc destination as operand 0 too
        self.writes = set()
        if self.op.startswith("v_cmpx"):
            self.writes = {("exec", 0)}
        elif self.op.startswith("v_") and self.opregs:
            self.writes = set(self.opregs[0])
            if self.op.startswith(_TWO_DEST) and len(self.opregs) > 1:
                self.writes |= self.opregs[1]

    @property
    def mfma_shape(self):
        m = re.match(r"v_mfma_[a-z0-9]+?_(\d+x\d+x\d+)_?([a-z0-9_]+)$", self.op)
        return f"{m.group(1)}_{m.group(2)}" if m else self.op

    def __repr__(self):
        return f"{self.line}: {self.text}"


class Kernel:
    def __init__(self, name):
        self.name, self.ins = name, []


def parse(text):
    """the functions of an assembly file: instructions with inline flags and static successor edges"""
    kernels, cur, labels, inline, block = [], None, {}, False, 0
    funcs = set(re.findall(r"^\s*\.type\s+([\w.$]+),@function", text, re.M))
    pending = []
    for ln, raw in enumerate(text.split("\n"), 1):
        s = raw.strip()
        if s.startswith(";;#ASMSTART"):
            inline, block = True, block + 1
            continue
        if s.startswith(";;#ASMEND"):
            inline = False
            continue
        s = s.split(";", 1)[0].split("//", 1)[0].strip()
        if not s:
            continue
        m = _LABEL.match(s)
        if m:
            name = m.group(1)
            if name in funcs:
                cur = Kernel(name); kernels.append(cur); labels = cur.labels = {}; pending = []
            elif name.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None:
                pending.append(name)
            s = s[m.end():].strip()
            if not s:
                continue
        if cur is None or s.startswith("."):
            continue
        for sub in s.split("\n"):
            ins = Instr(ln, sub.strip(), inline, block if inline else 0)
            for name in pending:
                labels[name] = len(cur.ins)
            pending = []
            cur.ins.append(ins)
    for k in kernels:
        n = len(k.ins)
        for i, ins in enumerate(k.ins):
            op = ins.op
            if op in ("s_endpgm", "s_setpc_b64", "s_trap") or op.startswith("s_endpgm"):
                continue
            if op == "s_branch" or op.startswith("s_cbranch"):
                t = k.labels.get(ins.ops[0]) if ins.ops else None
                if t is not None and t < n:
                    ins.succ.append(t)
                if op == "s_branch":
                    continue
            if i + 1 < n:
                ins.succ.append(i + 1)
    return kernels


def basic_blocks(k):
    """leaders of the kernel's basic blocks (labels that are branch targets, and what follows a branch)"""
    lead = {0}
    for i, ins in enumerate(k.ins):
        if ins.op == "s_branch" or ins.op.startswith("s_cbranch") or not ins.succ:
            lead.add(i + 1)
            lead.update(ins.succ)
    return sorted(x for x in lead if x < len(k.ins))


def walk(k, start, limit):
    """Every instruction reachable from behind k.ins[start] over static successor edges, with the SMALLEST number of wait
    states between the two, while that number is below `limit`.  Yields (index, states); the caller sends True to stop
    following the path behind an instruction."""
    best = {}
    todo = [(s, 0) for s in k.ins[start].succ]
    while todo:
        i, d = todo.pop()
        if d >= limit or best.get(i, limit + 1) <= d:
            continue
        best[i] = d
        stop = yield i, d
        if stop:
            continue
        nd = d + k.ins[i].states
        for s in k.ins[i].succ:
            todo.append((s, nd))


def _mfma_parts(ins):
    d = ins.opregs[0]
    a, b = ins.opregs[1], ins.opregs[2]
    c = ins.opregs[3] if len(ins.opregs) > 3 else set()
    return d, a, b, c


def h1_sites(k):
    """For every MFMA of the kernel: (instruction, nearest non-chain toucher of D, states between) — toucher None if
    nothing touches D within H1_LOOKAHEAD states.  The smallest distance per consumer is kept (a path found later may
    be shorter), so the walk is run to its end."""
    out = []
    for i, p in enumerate(k.ins):
        if not p.is_mfma:
            continue
        D = p.opregs[0]
        hit = {}
        chained = {}
        g = walk(k, i, H1_LOOKAHEAD)
        try:
            j, d = next(g)
            while True:
                c = k.ins[j]
                stop = False
                if c.regs & D:
                    stop = True
                    chain = False
                    if c.is_mfma:
                        cd, ca, cb, cc = _mfma_parts(c)
                        chain = cc == D and not ((ca | cb) & D)
                    if chain:
                        chained[j] = d
                    else:
                        hit[j] = min(d, hit.get(j, d))
                j, d = g.send(stop)
        except StopIteration:
            pass
        if hit:
            j = min(hit, key=lambda x: (hit[x], x))
            out.append((p, k.ins[j], hit[j]))
        else:
            out.append((p, None, None))
    return out


def _pairs(k, is_producer, written, is_consumer, read, limit):
    """generic producer -> consumer rule: consumers that read a register the producer wrote within `limit` states"""
    for i, p in enumerate(k.ins):
        if not is_producer(p):
            continue
        W = written(p)
        if not W:
            continue
        g = walk(k, i, limit)
        try:
            j, d = next(g)
            while True:
                c = k.ins[j]
                if is_consumer(c) and (read(c) & W):
                    yield p, c, d
                j, d = g.send(False)
        except StopIteration:
            pass                                    # this producer's paths are exhausted: on to the next one


def _vgprs(regs):
    return {r for r in regs if r[0] in ("v", "a")}


def _sgprs(regs):
    return {r for r in regs if r[0] in ("s", "vcc")}


def _is_vmem(i):
    return i.op.startswith("global_") or i.op.startswith("buffer_")


def scan_kernel(fname, k, h1_required):
    """(findings, statistics) of one kernel.  h1_required: shape -> states."""
    F, st = [], collections.OrderedDict()
    sites = h1_sites(k)
    st["mfma_inline"] = sum(1 for p, _, _ in sites if p.inline)
    st["mfma_builtin"] = sum(1 for p, _, _ in sites if not p.inline)
    for kind in ("inline", "builtin"):
        ds = [d for p, c, d in sites if c is not None and p.inline == (kind == "inline")]
        st[f"h1_min_{kind}"] = min(ds) if ds else None
    for p, c, d in sites:
        need = h1_required.get(p.mfma_shape)
        if c is not None and need is not None and d < need:
            F.append(Finding(fname, k.name, "H1", repr(p), repr(c), d, need))
    # H2, H3, H5: pairs are looked for a little beyond the requirement, so the report can say how near the nearest one
    # is (None: none that near)
    def rule(name, need, is_p, wr, is_c, rd):
        near = None
        for p, c, d in _pairs(k, is_p, wr, is_c, rd, need + RULE_LOOKAHEAD):
            near = d if near is None else min(near, d)
            if d < need:
                F.append(Finding(fname, k.name, name, repr(p), repr(c), d, need))
        st[name.lower() + "_min"] = near
    st["dpp"] = sum(1 for i in k.ins if i.is_dpp)
    rule("H2", H2_STATES, lambda i: i.is_valu, lambda i: _vgprs(i.writes), lambda i: i.is_dpp,
         lambda i: _vgprs(set().union(*i.opregs[1:]) if len(i.opregs) > 1 else set()))
    rule("H3", H3_STATES, lambda i: i.is_valu, lambda i: _sgprs(i.writes), _is_vmem, lambda i: _sgprs(i.regs))
    rule("H5", H5_STATES, lambda i: i.is_valu, lambda i: _vgprs(i.writes), lambda i: i.is_mfma and i.inline,
         lambda i: _vgprs(i.opregs[1] | i.opregs[2]))
    # H4
    dmas = [i for i, x in enumerate(k.ins) if x.op.startswith("global_load_lds")]
    m0w = {i for i, x in enumerate(k.ins) if x.op == "s_mov_b32" and x.ops[:1] == ["m0"]}
    other = [x for i, x in enumerate(k.ins) if ("m0", 0) in x.regs and i not in m0w]
    st["m0_writes"], st["m0_dma"], st["m0_other"] = len(m0w), len(dmas), len(other) if dmas else 0
    st["h4_min"] = None
    for i in dmas:
        x, ok, d, j = k.ins[i], False, 0, i - 1
        while x.inline and j >= 0 and k.ins[j].inline and k.ins[j].block == x.block:
            if j in m0w:
                ok = d >= H4_STATES
                st["h4_min"] = d if st["h4_min"] is None else min(st["h4_min"], d)
                break
            d += k.ins[j].states; j -= 1
        if not ok:
            F.append(Finding(fname, k.name, "H4", "s_mov_b32 m0 of the same asm block", repr(x), d if x.inline else 0, H4_STATES))
    if dmas:
        for x in other:
            F.append(Finding(fname, k.name, "H4", "a kernel with LDS-DMA", repr(x) + "  (m0 outside the DMA's asm)", 0, 0))
    uniq = {}
    for x in F:                                     # a consumer reached over two paths is one finding: the shorter
        key = (x.rule, x.producer, x.consumer)
        if key not in uniq or x.found < uniq[key].found:
            uniq[key] = x
    return list(uniq.values()), st, sites


def h1_table(all_sites):
    """shape -> (smallest distance behind a BUILTIN MFMA of that shape, number of builtin sites that attain it)"""
    by = collections.defaultdict(list)
    for p, c, d in all_sites:
        if not p.inline and c is not None:
            by[p.mfma_shape].append(d)
    return {s: (min(v), v.count(min(v))) for s, v in by.items()}


def inline_opcodes(kernels):
    """{opcode: [instructions]} over everything between ASMSTART and ASMEND"""
    out = collections.defaultdict(list)
    for k in kernels:
        for i in k.ins:
            if i.inline:
                out[i.op].append(i)
    return out


def allow_list_findings(fname, kernels):
    F = []
    for op, lst in inline_opcodes(kernels).items():
        for i in lst:
            if op not in INLINE_ALLOWED or not INLINE_ALLOWED[op](i):
                F.append(Finding(fname, "-", "allow-list", "inline assembly", repr(i), 0, 0))
                break
    return F


# ------------------------------------------------------------------------------------------------ compile the tree
def build_recipe():
    """(hipcc, flags, units) parsed from csrc/build.sh — the flags and the list of translation units that ship"""
    sh = open(os.path.join(CSRC, "build.sh")).read()
    flags = shlex.split(re.search(r'^FLAGS="([^"]*)"', sh, re.M).group(1).replace("$CFM_EXTRA_FLAGS", ""))
    units = re.search(r"^for f in ([\w ]+); do", sh, re.M).group(1).split()
    hipcc = os.environ.get("HIPCC") or re.search(r'HIPCC="\$\{HIPCC:-([^}]+)\}"', sh).group(1)
    return hipcc, flags, units


def _compile(args):
    hipcc, flags, src, out = args
    r = subprocess.run([hipcc, *flags, "-S", "--cuda-device-only", "-o", out, src], capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(f"{src}: {r.stderr[-2000:]}")
    return out


def compile_tree(outdir, jobs=MAX_JOBS):
    """every unit of build.sh -> outdir/<unit>.s, in parallel; returns {unit.hip: path}"""
    hipcc, flags, units = build_recipe()
    work = [(hipcc, flags, os.path.join(CSRC, u + ".hip"), os.path.join(outdir, u + ".s")) for u in units]
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(jobs, MAX_JOBS, len(work)))) as ex:
        paths = list(ex.map(_compile, work))
    return {u + ".hip": p for u, p in zip(units, paths)}


def audit(files, h1_required=None):
    """files: {display name: assembly path or text}.  Returns (findings, per-kernel statistics, measured H1 table).
    h1_required None: the measured table is its own requirement (the calibration: zero findings on compiler code)."""
    parsed, all_sites = {}, []
    for name, src in files.items():
        text = open(src).read() if "\n" not in src and os.path.exists(src) else src
        parsed[name] = parse(text)
    pre = {}
    for name, ks in parsed.items():
        for k in ks:
            pre[(name, k.name)] = h1_sites(k)
            all_sites += pre[(name, k.name)]
    table = h1_table(all_sites)
    need = h1_required if h1_required is not None else {s: v[0] for s, v in table.items()}
    findings, stats = [], collections.OrderedDict()
    for name, ks in parsed.items():
        findings += allow_list_findings(name, ks)
        for k in ks:
            F, st, _ = scan_kernel(name, k, need)
            findings += F
            stats[(name, k.name)] = st
    return findings, stats, table


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
        out = r.stdout.split("\n")
        return dict(zip(names, out)) if len(out) >= len(names) else {n: n for n in names}
    except OSError:
        return {n: n for n in names}


def format_report(findings, stats, table, seconds=None):
    L = ["# tools/isa_hazards.py — wait-state audit of the compiled kernels (see the tool's docstring for the rules)"]
    if seconds is not None:
        L.append(f"# compile (all units of build.sh, in parallel) {seconds[0]:.0f} s, scan {seconds[1]:.0f} s")
    L.append("# H1 table measured on the compiler's own (builtin) MFMA sites: shape -> smallest distance (sites attaining it)")
    for s, (d, n) in sorted(table.items()):
        L.append(f"#   {s}: {d} ({n} sites)")
    L.append(f"# H2 {H2_STATES}, H3 {H3_STATES}, H4 {H4_STATES}, H5 {H5_STATES} states")
    dm = demangle(sorted({k for _, k in stats}))
    cur = None
    for (f, k), st in stats.items():
        if not (st["mfma_inline"] or st["mfma_builtin"] or st["m0_dma"] or st["dpp"]):
            continue
        if f != cur:
            L.append(f"== {f}"); cur = f
        L.append(f"  mfma inline/builtin {st['mfma_inline']:4d}/{st['mfma_builtin']:4d}  H1 min inline/builtin "
                 f"{str(st['h1_min_inline']):>4s}/{str(st['h1_min_builtin']):>4s}  dpp {st['dpp']:3d} min H2/H3/H4/H5 "
                 f"{st['h2_min']}/{st['h3_min']}/{st['h4_min']}/{st['h5_min']}  m0 w/dma/other "
                 f"{st['m0_writes']}/{st['m0_dma']}/{st['m0_other']}  {dm[k][:100]}")
    L.append(f"findings: {len(findings)}")
    for x in findings:
        L.append(f"  {x.file} {dm.get(x.kernel, x.kernel)[:60]} {x.rule}: [{x.producer}] -> [{x.consumer}]  {x.found} < {x.required}")
    return "\n".join(L) + "\n"


def main(argv):
    out = None
    if "--out" in argv:
        i = argv.index("--out"); out = argv[i + 1]; argv = argv[:i] + argv[i + 2:]
    t0 = time.time()
    if argv:
        files, t1 = {os.path.basename(a): a for a in argv}, t0
        findings, stats, table = audit(files, H1_EXPECTED)
    else:
        with tempfile.TemporaryDirectory() as td:
            files = compile_tree(td)
            t1 = time.time()
            findings, stats, table = audit(files, H1_EXPECTED)
    rep = format_report(findings, stats, table, (t1 - t0, time.time() - t1))
    if out:
        open(out, "w").write(rep)
    sys.stdout.write(rep)
    return 1 if findings else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
