#!/usr/bin/env python3
"""Scan the gfx950 code of a built library for VALU-write -> MFMA-operand pairs that sit too close.

An MFMA that reads a register a vector-ALU instruction has just written needs two wait states between the two.  hipcc's
hazard recognizer pads the instructions it knows and does not look into inline-asm strings, so a pair whose producer
comes out of an asm statement is padded by luck or not at all, and no numerical test can tell (whether the MFMA takes
the stale register depends on issue timing, not on data).  This tool disassembles what was BUILT and measures the
distance:

    python tools/isa_hazards.py [whisper.tflite_amd/lib/libwhisper-tflite.so | file.o | file.co ...]

Extraction, with the tools of $ROCM_PATH/llvm/bin (default /opt/rocm): llvm-objcopy --dump-section .hip_fatbin (one
offload bundle per translation unit, back to back), clang-offload-bundler --unbundle for gfx950, llvm-objdump -d.
Temporaries go to a temporary directory; nothing is loaded into a process and nothing runs on a GPU.

The rule lives in RULES, one row per (producer class, consumer class, operand slots, states); a `Rule` with other
predicates adds another pair.  States between producer and consumer: `s_nop N` counts N + 1, every other instruction 1
(an `s_waitcnt` too: where it stalls the hazard is covered by accident, which is not credited).  Inside the window the
scan follows fall-through and, for `s_branch` / `s_cbranch_*`, the branch target as well; a label does not reset the
count.

Exit status 1 when there are violations, 2 when the extraction failed."""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile
from dataclasses import dataclass, field

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


class ToolError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------------------------------
# the rule table

_REG = re.compile(r"^([va])(?:(\d+)|\[(\d+):(\d+)\])$")


def parse_reg(op: str):
    """'v53' -> ('v', 53, 53); 'a[0:3]' -> ('a', 0, 3); anything else (SGPRs, constants, vcc, modifiers) -> None."""
    m = _REG.match(op)
    if not m:
        return None
    if m.group(2) is not None:
        return m.group(1), int(m.group(2)), int(m.group(2))
    return m.group(1), int(m.group(3)), int(m.group(4))


def _is_mfma(ins) -> bool:
    return "mfma" in ins.mnemonic


def _is_valu_non_mfma(ins) -> bool:
    return ins.mnemonic.startswith("v_") and not _is_mfma(ins)


def _valu_dests(ins):
    """The first operand is the destination (vN, v[a:b], a[..]; v_accvgpr_write's AGPR); the swaps write both of theirs."""
    n = 2 if "swap" in ins.mnemonic else 1
    return [r for r in (parse_reg(o) for o in ins.operands[:n]) if r]


@dataclass(frozen=True)
class Rule:
    name: str
    is_producer: object   # Instr -> bool
    dests: object         # Instr -> [(file, lo, hi)]
    is_consumer: object   # Instr -> bool
    slots: tuple          # ((operand index, slot name), ...) of the consumer
    states: int           # wait states required between producer and consumer


RULES = (
    # DESIGN section 24 / the kernel guide's "a just-written "v" operand or v_accvgpr_write -> MFMA operand (s_nop 1)"
    Rule("VALU write -> MFMA A/B/C", _is_valu_non_mfma, _valu_dests, _is_mfma, ((1, "A"), (2, "B"), (3, "C")), 2),
)


# ---------------------------------------------------------------------------------------------------------------------
# listings

@dataclass
class Instr:
    addr: int
    mnemonic: str
    operands: list
    text: str


@dataclass
class Kernel:
    symbol: str
    instrs: list = field(default_factory=list)


@dataclass
class Violation:
    rule: str
    kernel: str
    producer: Instr
    between: list
    consumer: Instr
    slot: str
    states: int

    def format(self) -> str:
        lines = [f"{self.kernel}", f"  {self.rule}: operand {self.slot} of the MFMA at {self.consumer.addr:#x} is read "
                 f"{self.states} state(s) behind its write"]
        for i in [self.producer] + self.between + [self.consumer]:
            lines.append(f"    {i.addr:8x}:  {i.text}")
        return "\n".join(lines)


@dataclass
class Report:
    kernels: int = 0
    kernels_with_mfma: int = 0
    mfmas: int = 0
    producers: int = 0
    symbols: list = field(default_factory=list)
    violations: list = field(default_factory=list)

    def merge(self, o: "Report") -> None:
        self.kernels += o.kernels
        self.kernels_with_mfma += o.kernels_with_mfma
        self.mfmas += o.mfmas
        self.producers += o.producers
        self.symbols += o.symbols
        self.violations += o.violations

    def format(self) -> str:
        out = [v.format() for v in self.violations]
        out.append(f"kernels scanned: {self.kernels} ({self.kernels_with_mfma} with an MFMA)   MFMAs seen: {self.mfmas}   "
                   f"producers checked: {self.producers}   violations: {len(self.violations)}")
        return "\n".join(out)


_SYM = re.compile(r"^[0-9a-fA-F]+ <(.+)>:\s*$")
_INS = re.compile(r"^\s+([a-z_][a-z0-9_]*)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")


def parse_listing(text: str):
    """llvm-objdump -d output -> [Kernel].  Lines that are neither a symbol nor an instruction are ignored."""
    kernels, cur = [], None
    for line in text.splitlines():
        if not line:
            continue
        if line[0] in " \t":
            m = _INS.match(line)
            if m and cur is not None:
                ops = [o.strip() for o in m.group(2).split(",")] if m.group(2) else []
                text_ = (m.group(1) + " " + m.group(2)).strip()
                cur.instrs.append(Instr(int(m.group(3), 16), m.group(1), ops, text_))
        else:
            m = _SYM.match(line)
            if m:
                cur = Kernel(m.group(1))
                kernels.append(cur)
    return kernels


def _cost(ins: Instr) -> int:
    if ins.mnemonic == "s_nop":
        return int(ins.operands[0], 0) + 1
    return 1


def _branch_target(ins: Instr):
    """Address an s_branch / s_cbranch_* jumps to: the dword behind the branch plus its signed 16-bit dword offset."""
    off = int(ins.operands[0].split()[0], 0) & 0xFFFF
    if off >= 0x8000:
        off -= 0x10000
    return ins.addr + 4 + 4 * off


def _overlap(a, b) -> bool:
    return a[0] == b[0] and a[1] <= b[2] and b[1] <= a[2]


def scan_kernel(k: Kernel, rules=RULES) -> Report:
    rep = Report(kernels=1, symbols=[k.symbol])
    ins = k.instrs
    rep.mfmas = sum(1 for i in ins if _is_mfma(i))
    if not rep.mfmas:
        return rep   # no consumer of any rule of the table: nothing to measure
    rep.kernels_with_mfma = 1
    index = {i.addr: n for n, i in enumerate(ins)}
    for rule in rules:
        for p, prod in enumerate(ins):
            if not rule.is_producer(prod):
                continue
            dests = rule.dests(prod)
            if not dests:
                continue
            rep.producers += 1
            # (index of the next instruction, states so far, instructions passed); the window is `states` wide, so the
            # walk ends after a few steps whatever the control flow
            work, seen = [(p + 1, 0, [])], set()
            while work:
                j, st, path = work.pop()
                if j >= len(ins) or (j, st) in seen:
                    continue
                seen.add((j, st))
                cur = ins[j]
                if rule.is_consumer(cur):
                    for slot, name in rule.slots:
                        r = parse_reg(cur.operands[slot]) if slot < len(cur.operands) else None
                        if r and any(_overlap(r, d) for d in dests):
                            rep.violations.append(Violation(rule.name, k.symbol, prod, path, cur, name, st))
                st2 = st + _cost(cur)
                if st2 >= rule.states:
                    continue
                m = cur.mnemonic
                if m in ("s_endpgm", "s_setpc_b64", "s_swappc_b64"):
                    continue
                if m == "s_branch" or m.startswith("s_cbranch"):
                    t = index.get(_branch_target(cur))
                    if t is not None:
                        work.append((t, st2, path + [cur]))
                    if m == "s_branch":
                        continue
                work.append((j + 1, st2, path + [cur]))
    return rep


def scan_listing(text: str, rules=RULES) -> Report:
    rep = Report()
    for k in parse_listing(text):
        rep.merge(scan_kernel(k, rules))
    return rep


# ---------------------------------------------------------------------------------------------------------------------
# from a built file to listings

def llvm_tool(name: str) -> str:
    path = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)
    if not os.path.exists(path):
        raise ToolError(f"{path} not found (ROCM_PATH?)")
    return path


def _run(cmd, **kw):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, **kw)
    if r.returncode != 0:
        raise ToolError(f"{' '.join(cmd)}: exit {r.returncode}: {r.stderr.decode(errors='replace').strip()}")
    return r.stdout


def code_objects(path: str, tmp: str):
    """Paths of the gfx950 code objects inside `path`: a shared library or host object with a .hip_fatbin section, an
    offload bundle, or a device code object itself (hipcc --cuda-device-only -c)."""
    with open(path, "rb") as f:
        data = f.read()
    base = os.path.join(tmp, os.path.basename(path))
    if data[:4] == b"\x7fELF" and data[18:20] == (224).to_bytes(2, "little"):  # e_machine EM_AMDGPU
        return [path]
    if data[:4] == b"\x7fELF":
        fat = base + ".fatbin"
        _run([llvm_tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", path, base + ".copy"])
        with open(fat, "rb") as f:
            data = f.read()
    starts = []
    at = data.find(BUNDLE_MAGIC)
    while at >= 0:
        starts.append(at)
        at = data.find(BUNDLE_MAGIC, at + 1)
    if not starts:
        raise ToolError(f"{path}: no offload bundle found")
    out = []
    for n, s in enumerate(starts):
        piece, co = f"{base}.{n}.bundle", f"{base}.{n}.co"
        with open(piece, "wb") as f:
            f.write(data[s:starts[n + 1] if n + 1 < len(starts) else len(data)])
        _run([llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={piece}",
              f"--output={co}"])
        if os.path.getsize(co) == 0:
            raise ToolError(f"{path}: bundle {n} holds no {TARGET} code object")
        out.append(co)
    return out


def demangle(symbols):
    try:
        tool = llvm_tool("llvm-cxxfilt")
    except ToolError:
        return {s: s for s in symbols}
    out = _run([tool], input="\n".join(symbols).encode()).decode().splitlines()
    return dict(zip(symbols, out)) if len(out) == len(symbols) else {s: s for s in symbols}


def scan_file(path: str, rules=RULES) -> Report:
    rep = Report()
    with tempfile.TemporaryDirectory(prefix="isa_hazards_") as tmp:
        for co in code_objects(path, tmp):
            rep.merge(scan_listing(_run([llvm_tool("llvm-objdump"), "-d", co]).decode(), rules))
    names = demangle(rep.symbols)
    rep.symbols = [names[s] for s in rep.symbols]
    for v in rep.violations:
        v.kernel = names.get(v.kernel, v.kernel)
    return rep


def default_library() -> str:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return os.path.join(root, "whisper.tflite_amd", "lib", "libwhisper-tflite.so")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("files", nargs="*", help="shared library, object or code object (default: the built library)")
    args = ap.parse_args(argv)
    total = Report()
    try:
        for f in args.files or [default_library()]:
            total.merge(scan_file(f))
    except (ToolError, OSError) as e:
        print(f"isa_hazards: {e}", file=sys.stderr)
        return 2
    print(total.format())
    return 1 if total.violations else 0


if __name__ == "__main__":
    sys.exit(main())
