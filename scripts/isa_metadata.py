"""Register / LDS / spill metadata of every kernel in libpgmi.so's sources, from hipcc's own assembly (gfx950 code-object notes).

    python scripts/isa_metadata.py > profiles/r3/isa_metadata.txt        # no GPU needed (hipcc cross-compiles)

Columns: arch VGPRs, AGPRs, SGPRs, SGPR / VGPR spills, scratch bytes per lane, static LDS bytes, MFMA instructions in the body; then,
to compare the code generation of two trees with `diff`: the instruction count, a hash of the instruction stream (comments dropped,
block labels numbered within the kernel, the kernarg offset of the scalar argument loads `s_load_* s[..], s[0:1], 0x..` masked: an
argument added or removed in front moves it and nothing else) and a hash of the opcode histogram without s_nop (equal when the compiler
only ordered the same instructions differently or numbered registers differently)."""
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from proteingym_amd import build_native as bn  # noqa: E402


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def stream_columns(body):
    """(instruction count, stream hash, opcode-histogram hash) of one kernel's assembly text."""
    lines = []
    for ln in body.split("\n"):
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0]).strip()       # the label prefix numbers the kernel within its file
        if ln and not ln.startswith("."):                                  # directives; block labels start with '.' too
            lines.append(re.sub(r"^(s_load_\S+\s+s\[?[\d:]+\]?, s\[0:1\], )0x[0-9a-f]+", r"\1<kernarg>", " ".join(ln.split())))
        elif ln.endswith(":"):
            lines.append(ln)
    ins = [ln.split()[0] for ln in lines if not ln.endswith(":")]
    hist = sorted(collections.Counter(op for op in ins if op != "s_nop").items())
    short = lambda t: hashlib.sha256(t.encode()).hexdigest()[:10]  # noqa: E731
    return len(ins), short("\n".join(lines)), short(repr(hist))


def main():
    print(f"build digest {bn._digest()[:16]}  flags: {' '.join(bn.FLAGS)}")
    with tempfile.TemporaryDirectory() as d:
        for src in bn.SOURCES:
            asm = os.path.join(d, src + ".s")
            subprocess.run([bn._hipcc(), *bn.FLAGS, *bn.EXTRA_FLAGS.get(src, []), "-S", "--cuda-device-only", "-w",
                            os.path.join(bn.CSRC, src), "-o", asm], check=True, capture_output=True)
            text = open(asm).read()
            mfma, stream = {}, {}
            for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)\n\s*s_endpgm", text, re.S | re.M):
                mfma[m.group(1)] = len(re.findall(r"^\s*v_mfma", m.group(2), re.M))
            for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)\n\.Lfunc_end\d+:", text, re.S | re.M):      # the whole body: an early exit has its own s_endpgm
                stream[m.group(1)] = stream_columns(m.group(2))
            kernels = re.findall(r"- \.agpr_count:.*?\.wavefront_size:\s*\d+", text, re.S)
            rows = []
            for k in kernels:
                g = lambda key: (re.search(rf"\.{key}:\s*(\S+)", k) or [None, "?"])[1]  # noqa: E731
                rows.append((g("name"), g("vgpr_count"), g("agpr_count"), g("sgpr_count"), g("sgpr_spill_count"), g("vgpr_spill_count"),
                             g("private_segment_fixed_size"), g("group_segment_fixed_size")))
            names = demangle([r[0] for r in rows])
            print(f"\n== {src}")
            print(f"{'VGPR':>5} {'AGPR':>5} {'SGPR':>5} {'sSpill':>6} {'vSpill':>6} {'scratch':>7} {'LDS':>7} {'MFMA':>5} {'instr':>6} {'stream':>10} {'opcodes':>10}  kernel")
            for r in rows:
                nm = re.sub(r"\(.*", "", names.get(r[0], r[0]))
                n, h_stream, h_ops = stream.get(r[0], (0, "?", "?"))
                print(f"{r[1]:>5} {r[2]:>5} {r[3]:>5} {r[4]:>6} {r[5]:>6} {r[6]:>7} {r[7]:>7} {mfma.get(r[0], 0):>5} {n:>6} {h_stream:>10} {h_ops:>10}  {nm}")


if __name__ == "__main__":
    main()
