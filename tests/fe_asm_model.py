"""A CPU model of the generated device code of the field products: csrc/fe25519_gen.inc, read as the compiler reads it, its asm
templates executed instruction by instruction on Python integers.

Two kinds of code live in that file.  The per-column helpers act_cz* / act_c* exist twice, as an asm statement under
__HIP_DEVICE_COMPILE__ and as a C expression in the #else branch; the host tests run the second only.  The one-statement products
ACT_FE_*_ONE_ASM exist only as asm on the fixed registers v232..v254 and run only in the range kernel's translation unit.  This
module parses both (helpers(), macro()), runs a template (run_helper(), run_macro()), and evaluates a host twin's expression
(eval_host_helper()).

The model does not guess.  An unknown mnemonic, an operand it cannot read, an operand list of the wrong length or a literal the
encoding has no room for raise ModelError; so do
  * a v_mad_u64_u32 whose exact sum does not fit 64 bits, a v_add_u32 that wraps, a v_mul_u32_u24 operand of 2^24 or more,
  * a 32-bit wrap in a macro's C prelude (`const uint32_t x = 2u * f.v[i]`),
  * a fixed register read before the statement wrote it, or written without being on the clobber list,
  * an output operand read before it is written, an input operand written, and a write to an output that is not early-clobber
    while inputs are still to be read (the compiler may have put an input there).
It uses nothing but the text: tools/gen_fe_mul.py is not imported."""
import os
import re

GEN_INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "anonymous-credit-tokens_amd", "csrc", "fe25519_gen.inc")
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
ONE_ASM_MACROS = ("ACT_FE_MUL_ONE_ASM", "ACT_FE_SQ_ONE_ASM", "ACT_FE_MUL2_ONE_ASM", "ACT_FE_SQ2_ONE_ASM", "ACT_FE_SQDA_SQ_ONE_ASM")


class ModelError(Exception):
    pass


def source(path=GEN_INC):
    with open(path) as f:
        return f.read()


# ---- C side: asm statements, operand lists, preludes ----------------------------------------------------------------------------
class Operand:
    def __init__(self, name, constraint, expr):
        self.name, self.constraint, self.expr = name, constraint, expr
        self.is_output = constraint[0] in "=+"
        self.reads_first = constraint[0] == "+"
        self.early = "&" in constraint
        self.scalar = constraint.lstrip("=+&") == "s"
        if constraint.lstrip("=+&") not in ("v", "s"):
            raise ModelError("constraint %r of operand %r: only \"v\" and \"s\" are modelled" % (constraint, expr))


class Statement:
    """One asm statement: its instructions, operands (outputs first, as %N counts them) and clobbered fixed registers."""
    def __init__(self, instructions, operands, clobbers):
        self.instructions, self.operands, self.clobbers = instructions, operands, clobbers
        self.by_name = {o.name: i for i, o in enumerate(operands) if o.name}


def _split_top(s, sep):
    """Split at `sep` outside string literals, parentheses and brackets."""
    out, depth, quote, cur, i = [], 0, False, [], 0
    while i < len(s):
        c = s[i]
        if quote:
            cur.append(c)
            if c == "\\":
                cur.append(s[i + 1]); i += 1
            elif c == '"':
                quote = False
        elif c == '"':
            quote = True; cur.append(c)
        elif c in "([":
            depth += 1; cur.append(c)
        elif c in ")]":
            depth -= 1; cur.append(c)
        elif c == sep and depth == 0:
            out.append("".join(cur)); cur = []
        else:
            cur.append(c)
        i += 1
    out.append("".join(cur))
    return out


def _unescape(s):
    return s.replace("\\n", "\n").replace("\\t", "\t")


def parse_asm(text):
    """`asm("..." "..." : outputs : inputs : clobbers);` somewhere in `text` -> (Statement, text before it, text after it)."""
    m = re.search(r"\basm\s*\(", text)
    if not m:
        raise ModelError("no asm statement found")
    depth, i, quote = 1, m.end(), False
    while depth:
        if i >= len(text):
            raise ModelError("asm statement does not close")
        c = text[i]
        if quote:
            if c == "\\":
                i += 1
            elif c == '"':
                quote = False
        elif c == '"':
            quote = True
        elif c == "(":
            depth += 1
        elif c == ")":
            depth -= 1
        i += 1
    parts = _split_top(text[m.end():i - 1], ":")
    if len(parts) != 4:
        raise ModelError("asm statement: expected template : outputs : inputs : clobbers, found %d sections" % len(parts))
    pieces = re.findall(r'"((?:[^"\\]|\\.)*)"', parts[0])
    if re.sub(r'"((?:[^"\\]|\\.)*)"', "", parts[0]).strip():
        raise ModelError("asm template: text between the string literals: %r" % re.sub(r'"((?:[^"\\]|\\.)*)"', "", parts[0]).strip()[:40])
    instructions = [l.strip() for l in _unescape("".join(pieces)).split("\n") if l.strip()]
    operands = []
    for section, want_output in ((parts[1], True), (parts[2], False)):
        for item in _split_top(section, ","):
            item = item.strip()
            if not item:
                continue
            mo = re.fullmatch(r'(?:\[(\w+)\]\s*)?"([^"]+)"\s*\((.*)\)', item, re.S)
            if not mo:
                raise ModelError("operand %r not understood" % item)
            op = Operand(mo.group(1), mo.group(2), mo.group(3).strip())
            if op.is_output != want_output:
                raise ModelError("operand %r is in the wrong list" % item)
            operands.append(op)
    clobbers = set()
    for item in _split_top(parts[3], ","):
        mo = re.fullmatch(r'\s*"(\w+)"\s*', item)
        if not mo:
            raise ModelError("clobber %r not understood" % item)
        clobbers.add(mo.group(1))
    return Statement(instructions, operands, clobbers), text[:m.start()], text[i:]


class Helper:
    def __init__(self, name, params, body):
        self.name, self.params, self.body = name, params, body      # params: [(type, name)], the accumulator first


def helpers(text):
    """The per-column helpers of both branches: ({name: Helper} of the device branch, {name: Helper} of the host branch)."""
    m = re.search(r"^#if defined\(__HIP_DEVICE_COMPILE__\)\n(.*?)^#else\n(.*?)^#endif\n", text, re.S | re.M)
    if not m:
        raise ModelError("no #if defined(__HIP_DEVICE_COMPILE__) / #else / #endif block of helpers")
    out = []
    for branch in (m.group(1), m.group(2)):
        d = {}
        for line in branch.splitlines():
            if not line.strip():
                continue
            mo = re.fullmatch(r"static (?:__device__ __forceinline__|inline) void (\w+)\(([^)]*)\) \{ (.*) \}", line.strip())
            if not mo:
                raise ModelError("helper line not understood: %r" % line[:80])
            params = []
            for p in mo.group(2).split(","):
                mp = re.fullmatch(r"\s*(uint64_t&|uint32_t) (\w+)\s*", p)
                if not mp:
                    raise ModelError("%s: parameter %r not understood" % (mo.group(1), p))
                params.append((mp.group(1), mp.group(2)))
            if mo.group(1) in d:
                raise ModelError("helper %s defined twice in one branch" % mo.group(1))
            d[mo.group(1)] = Helper(mo.group(1), params, mo.group(3))
        out.append(d)
    return out[0], out[1]


def macro(text, name):
    """Body of `#define name \\` with its continuation lines joined."""
    m = re.search(r"^#define %s \\\n((?:.*\\\n)*.*\n)" % re.escape(name), text, re.M)
    if not m:
        raise ModelError("macro %s not found" % name)
    return m.group(1).replace("\\\n", "\n")


def _c_value(expr, env):
    """An input operand's C expression: x, x.v[i] or a literal."""
    e = expr.strip()
    mo = re.fullmatch(r"(\w+)\.v\[(\d+)\]", e)
    if mo:
        if mo.group(1) not in env:
            raise ModelError("operand %r: no value for %r" % (e, mo.group(1)))
        return env[mo.group(1)][int(mo.group(2))]
    if re.fullmatch(r"\d+u?", e):
        return int(e.rstrip("u"))
    if re.fullmatch(r"0x[0-9a-fA-F]+u?", e):
        return int(e.rstrip("u"), 16)
    if re.fullmatch(r"[A-Za-z_]\w*", e):
        if e not in env:
            raise ModelError("operand %r has no value" % e)
        return env[e]
    raise ModelError("C expression %r not understood" % e)


def _prelude(text, env, allow_wrap):
    """`const uint32_t x = 2u * f.v[1], y = ...;` declarations into env; returns the names whose product wrapped 32 bits."""
    wraps = []
    rest = text.strip()
    while rest:
        mo = re.match(r"const uint32_t ([^;]*);", rest)
        if not mo:
            raise ModelError("prelude not understood: %r" % rest[:60])
        for decl in mo.group(1).split(","):
            md = re.fullmatch(r"\s*(\w+) = (\d+)u \* (\w+\.v\[\d+\])\s*", decl)
            if not md:
                raise ModelError("prelude declaration %r not understood" % decl)
            v = int(md.group(2)) * _c_value(md.group(3), env)
            if v > M32:
                wraps.append(md.group(1))
                if not allow_wrap:
                    raise ModelError("prelude: %s = %s wraps 32 bits" % (md.group(1), decl.split("=", 1)[1].strip()))
            env[md.group(1)] = v & M32
        rest = rest[mo.end():].strip()
    return wraps


# ---- the instructions -----------------------------------------------------------------------------------------------------------
class Report:
    """results: {variable: its nine raw limbs} of a macro, or {"acc": value} of a helper; max_column: the largest 64-bit value a
    multiply-accumulate produced; instructions: how many the statement holds; wraps: prelude names that wrapped (allow_wrap only)."""
    def __init__(self):
        self.results, self.max_column, self.instructions, self.wraps = {}, 0, 0, []


class _Machine:
    def __init__(self, st, in_values, inout_values):
        self.st = st
        self.regs = {}                                  # fixed VGPR number -> 32-bit value, written ones only
        self.val = {}                                   # operand index -> value
        self.width = {}                                 # operand index -> 32 / 64 once it has a value
        self.first_write, self.last_read = {}, {}
        self.pc = 0
        self.max_column = 0
        for i, o in enumerate(st.operands):
            if not o.is_output:
                self.val[i] = in_values[i]; self.width[i] = 32
            elif o.reads_first:
                self.val[i] = inout_values[i]; self.width[i] = 64 if inout_values[i] > M32 else None

    def err(self, msg):
        raise ModelError("instruction %d `%s`: %s" % (self.pc, self.st.instructions[self.pc], msg))

    def _operand_index(self, tok):
        mo = re.fullmatch(r"%\[(\w+)\]", tok)
        if mo:
            if mo.group(1) not in self.st.by_name:
                self.err("no operand named %s" % mo.group(1))
            return self.st.by_name[mo.group(1)]
        mo = re.fullmatch(r"%(\d+)", tok)
        if mo:
            if int(mo.group(1)) >= len(self.st.operands):
                self.err("no operand %s" % tok)
            return int(mo.group(1))
        return None

    def _literal(self, tok):
        if re.fullmatch(r"\d+", tok):
            return int(tok)
        if re.fullmatch(r"0x[0-9a-fA-F]+", tok):
            return int(tok, 16)
        return None

    def _fixed(self, n, what):
        if n not in self.regs:
            self.err("v%d is %s before this statement wrote it" % (n, what))
        return self.regs[n]

    def read(self, tok, bits, inline_only):
        """Value of a source operand of `bits` bits.  inline_only: the encoding (VOP3) has no literal, only the inline constants 0..64."""
        lit = self._literal(tok)
        if lit is not None:
            if inline_only and lit > 64:
                self.err("literal %s is no inline constant (0..64) and this encoding takes no literal" % tok)
            if lit > M32:
                self.err("literal %s exceeds 32 bits" % tok)
            return lit
        i = self._operand_index(tok)
        if i is not None:
            if i not in self.val:
                self.err("output operand %s read before it is written" % tok)
            if self.width[i] is not None and self.width[i] != bits:
                self.err("operand %s holds %d bits, read as %d" % (tok, self.width[i], bits))
            if not self.st.operands[i].is_output or self.st.operands[i].reads_first:
                self.last_read[i] = self.pc
            return self.val[i]
        mo = re.fullmatch(r"v(\d+)", tok)
        if mo and bits == 32:
            return self._fixed(int(mo.group(1)), "read")
        mo = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
        if mo and bits == 64:
            lo, hi = int(mo.group(1)), int(mo.group(2))
            if hi != lo + 1:
                self.err("register range %s is not a pair" % tok)
            return self._fixed(lo, "read") | (self._fixed(hi, "read") << 32)
        self.err("source operand %r (%d bits) not understood" % (tok, bits))

    def write(self, tok, bits, value):
        assert 0 <= value < (1 << bits)
        i = self._operand_index(tok)
        if i is not None:
            if not self.st.operands[i].is_output:
                self.err("input operand %s written" % tok)
            if self.st.operands[i].scalar:
                self.err("vector result written to the scalar operand %s" % tok)
            self.val[i] = value; self.width[i] = bits
            self.first_write.setdefault(i, self.pc)
            return
        regs = None
        mo = re.fullmatch(r"v(\d+)", tok)
        if mo and bits == 32:
            regs = [int(mo.group(1))]
        mo = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
        if mo and bits == 64:
            if int(mo.group(2)) != int(mo.group(1)) + 1:
                self.err("register range %s is not a pair" % tok)
            regs = [int(mo.group(1)), int(mo.group(1)) + 1]
        if regs is None:
            self.err("destination %r (%d bits) not understood" % (tok, bits))
        for k, n in enumerate(regs):
            if "v%d" % n not in self.st.clobbers:
                self.err("v%d is written but is not on the clobber list" % n)
            self.regs[n] = (value >> (32 * k)) & M32

    def step(self):
        line = self.st.instructions[self.pc]
        mnemonic, _, rest = line.partition(" ")
        a = [t.strip() for t in rest.split(",")]

        def arity(n):
            if len(a) != n:
                self.err("%s takes %d operands, found %d" % (mnemonic, n, len(a)))
        if mnemonic == "v_mad_u64_u32":
            arity(5)
            if a[1] != "vcc":
                self.err("carry-out goes to %r, not vcc" % a[1])
            if "vcc" not in self.st.clobbers:
                self.err("vcc is written but is not on the clobber list")
            scalars = [t for t in a[2:4] if self._operand_index(t) is not None and self.st.operands[self._operand_index(t)].scalar]
            if len(scalars) > 1:
                self.err("two scalar-register sources in one VOP3 instruction")
            s = self.read(a[2], 32, True) * self.read(a[3], 32, True) + self.read(a[4], 64, True)
            if s > M64:
                self.err("the sum needs %d bits: the column overflows 2^64" % s.bit_length())
            self.max_column = max(self.max_column, s)
            self.write(a[0], 64, s)
        elif mnemonic == "v_lshrrev_b64":
            arity(3)
            self.write(a[0], 64, self.read(a[2], 64, True) >> (self.read(a[1], 32, True) & 63))
        elif mnemonic == "v_lshrrev_b32":
            arity(3)
            self.write(a[0], 32, self.read(a[2], 32, False) >> (self.read(a[1], 32, False) & 31))
        elif mnemonic == "v_alignbit_b32":
            arity(4)
            self.write(a[0], 32, (((self.read(a[1], 32, True) << 32) | self.read(a[2], 32, True)) >> (self.read(a[3], 32, True) & 31)) & M32)
        elif mnemonic == "v_and_b32":
            arity(3)
            self.write(a[0], 32, self.read(a[1], 32, False) & self.read(a[2], 32, False))
        elif mnemonic == "v_add_u32":
            arity(3)
            s = self.read(a[1], 32, False) + self.read(a[2], 32, False)
            if s > M32:
                self.err("the 32-bit sum wraps")
            self.write(a[0], 32, s)
        elif mnemonic == "v_mul_u32_u24":
            arity(3)
            x, y = self.read(a[1], 32, False), self.read(a[2], 32, False)
            if x >> 24 or y >> 24:
                self.err("an operand of %d bits: v_mul_u32_u24 multiplies the low 24 only" % max(x.bit_length(), y.bit_length()))
            if x * y > M32:
                self.err("the product exceeds 32 bits")
            self.write(a[0], 32, x * y)
        else:
            self.err("mnemonic %r is not modelled" % mnemonic)
        self.pc += 1

    def run(self):
        while self.pc < len(self.st.instructions):
            self.step()
        # an output that is not early-clobber may share a register with an input: every input must have been read before it is written
        reads = [self.last_read.get(i, -1) for i, o in enumerate(self.st.operands) if not o.is_output]
        for i, o in enumerate(self.st.operands):
            if o.is_output and not o.early and not o.reads_first and i in self.first_write and reads and self.first_write[i] < max(reads):
                raise ModelError("output operand %d (%s) is written at instruction %d while inputs are still to be read, and is not early-clobber" %
                                 (i, o.expr, self.first_write[i]))
            if o.is_output and i not in self.first_write:
                raise ModelError("output operand %d (%s) is never written" % (i, o.expr))


def _execute(st, env, inout_exprs):
    ins, inouts = {}, {}
    for i, o in enumerate(st.operands):
        if not o.is_output:
            v = _c_value(o.expr, env)
            if not 0 <= v <= M32:
                raise ModelError("input %s = %d does not fit a 32-bit register" % (o.expr, v))
            ins[i] = v
        elif o.reads_first:
            inouts[i] = inout_exprs[o.expr]
    mach = _Machine(st, ins, inouts)
    mach.run()
    return mach


def run_macro(text, name, allow_wrap=False, **operands):
    """Run one ACT_FE_*_ONE_ASM statement of `text` on the named nine-limb operands (f, g, fb, gb, a: what the macro reads)."""
    st, before, after = parse_asm(macro(text, name))
    if after.strip(" ;\n"):
        raise ModelError("%s: text after the asm statement: %r" % (name, after.strip()[:40]))
    env = {k: list(v) for k, v in operands.items()}
    for k, v in env.items():
        if len(v) != 9 or any(not 0 <= l <= M32 for l in v):
            raise ModelError("operand %s: nine 32-bit limbs wanted" % k)
    rep = Report()
    rep.wraps = _prelude(before, env, allow_wrap)
    mach = _execute(st, env, {})
    for i, o in enumerate(st.operands):
        if o.is_output:
            mo = re.fullmatch(r"(\w+)\.v\[(\d+)\]", o.expr)
            if not mo or mach.width[i] != 32:
                raise ModelError("%s: output %r is not a limb" % (name, o.expr))
            limbs = rep.results.setdefault(mo.group(1), [None] * 9)
            if limbs[int(mo.group(2))] is not None:
                raise ModelError("%s: limb %s bound to two outputs" % (name, o.expr))
            limbs[int(mo.group(2))] = mach.val[i]
    for k, limbs in rep.results.items():
        if None in limbs:
            raise ModelError("%s: %s.v[%d] is not an output" % (name, k, limbs.index(None)))
    rep.max_column, rep.instructions = mach.max_column, len(st.instructions)
    return rep


def run_helper(h, acc, args):
    """Run a device-branch helper's asm statement: acc = the accumulator on entry (ignored by the act_cz* forms, which start from
    zero), args = the uint32_t arguments in order.  results["acc"] is the accumulator on return."""
    st, before, after = parse_asm(h.body)
    if before.strip() or after.strip(" ;"):
        raise ModelError("%s: text around the asm statement" % h.name)
    if h.params[0] != ("uint64_t&", "acc") or any(t != "uint32_t" for t, _ in h.params[1:]) or len(args) != len(h.params) - 1:
        raise ModelError("%s: wants (uint64_t& acc, uint32_t ...) and %d arguments" % (h.name, len(h.params) - 1))
    env = dict((n, v) for (_, n), v in zip(h.params[1:], args))
    mach = _execute(st, env, {"acc": acc})
    outs = [i for i, o in enumerate(st.operands) if o.is_output]
    if len(outs) != 1 or st.operands[outs[0]].expr != "acc" or mach.width[outs[0]] != 64:
        raise ModelError("%s: the one output must be the 64-bit accumulator" % h.name)
    rep = Report()
    rep.results["acc"], rep.max_column, rep.instructions = mach.val[outs[0]], mach.max_column, len(st.instructions)
    return rep


def eval_host_helper(h, acc, args):
    """The host twin's `acc = [acc +] (uint64_t)x * (uint64_t)y + ...;` as C computes it: modulo 2^64."""
    mo = re.fullmatch(r"acc = (.*);", h.body.strip())
    if not mo or len(args) != len(h.params) - 1:
        raise ModelError("%s: host body %r not understood" % (h.name, h.body[:60]))
    env = dict((n, v) for (_, n), v in zip(h.params[1:], args))
    env["acc"] = acc
    total = 0
    for term in mo.group(1).split(" + "):
        if term == "acc":
            total += env["acc"]
            continue
        mt = re.fullmatch(r"\(uint64_t\)(\w+) \* \(uint64_t\)(\w+)", term)
        if not mt:
            raise ModelError("%s: host term %r not understood" % (h.name, term))
        total += _c_value(mt.group(1), env) * _c_value(mt.group(2), env)
    return total & M64
