#!/usr/bin/env python3
"""Per-kernel resources of the library's HIP kernels, from the compiler alone (no GPU is needed).

Compiles the kernel files to device assembly with the library's flags and prints, per kernel: VGPRs, SGPRs, LDS bytes,
scratch bytes, spilled registers (vector + scalar) and the number of instruction lines of the kernel's body.  The numbers
are the code object's own metadata (the amdhsa.kernels note); the instruction lines are counted, not classified.

  python tools/kernel_resources.py                       # every kernel of every .hip file the library is built from
  python tools/kernel_resources.py --match k_render      # kernels whose demangled name contains the text
  python tools/kernel_resources.py --json out.json -DVH_RENDER_WAVES=5 vh_kernels.hip vh_icp.hip
  python tools/kernel_resources.py --against ../parent/voxelhashing_amd/csrc    # what a refactor did to each kernel

--against DIR compiles the same-named sources of another checkout's csrc as well (or all its .hip files when no sources
are given: kernels may have moved between files) and says per kernel whether its instruction sequence -- comments,
directives, labels and the numbers of local labels aside -- is identical, differs, or exists on one side only.

Every file is compiled with the flags the library's build gives it (`build.flags(source)`: the common flags and the extra
ones of `build.SOURCE_FLAGS` by file name), the other checkout's files with this checkout's flags: --against compares
sources, like with like.  (What the other checkout's own build makes of them, its own copy of this tool says.)

`resources(asm_text)`, `instruction_sequences(asm_text)` and `library_resources(lib)` are importable: the last reads the
same metadata out of a built library (tests/test_kernel_resources.py).
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIELDS = (("vgprs", ".vgpr_count"), ("sgprs", ".sgpr_count"), ("lds_bytes", ".group_segment_fixed_size"),
          ("scratch_bytes", ".private_segment_fixed_size"), ("vgpr_spills", ".vgpr_spill_count"),
          ("sgpr_spills", ".sgpr_spill_count"))


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    for cand in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"):
        if tool is None and os.path.exists(cand):
            tool = cand
    if tool is None or not names:
        return {n: n for n in names}
    out = subprocess.run([tool] + list(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {n: re.sub(r"^void ", "", d).replace("(anonymous namespace)::", "") for n, d in zip(names, out)}


def metadata_kernels(text):
    """[{name, vgprs, ...}] from the YAML of an amdhsa.kernels note (as it stands in device assembly or in a note section)."""
    kernels = []
    start = text.find("amdhsa.kernels:")
    if start < 0:
        return kernels
    # every kernel's mapping starts with "  - .agpr_count:" (keys are sorted) at the list's own indentation
    body = text[start:]
    end = body.find("amdhsa.target:")
    if end >= 0:
        body = body[:end]
    for item in re.split(r"\n  - (?=\.)", body)[1:]:
        k = {}
        for line in item.split("\n"):
            m = re.match(r"^\s{4}(\.[a-z_]+):\s*(\S.*)$", "    " + line if not line.startswith(" ") else line)
            if m and m.group(1) not in k:
                k[m.group(1)] = m.group(2).strip().strip("'\"")
        if ".name" not in k:
            continue
        row = {"name": k[".name"]}
        for out, key in FIELDS:
            row[out] = int(k.get(key, "0"), 0)
        kernels.append(row)
    return kernels


def instruction_lines(text, name):
    """instruction lines between the kernel's label and the end of its body"""
    m = re.search(r"^" + re.escape(name) + r":\s*(;.*)?$", text, re.M)
    if not m:
        return 0
    end = re.compile(r"^\s*(\.Lfunc_end\d+:|\.section\b|\.amdhsa_kernel\b)")
    n = 0
    for line in text[m.end():].split("\n"):
        if end.match(line):
            break
        s = line.strip()
        if not s or s[0] in ".;" or s.endswith(":") or re.match(r"^\S+:\s*(;.*)?$", s):
            continue
        n += 1
    return n


def instruction_sequences(asm_text):
    """{mangled kernel name: [instruction lines]} of every kernel, weak (template) ones included: the lines between the
    kernel's label and the end of its body, without comments, directives and labels, local label numbers blanked"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm_text, re.M)
    end = re.compile(r"^\s*(\.Lfunc_end\d+:|\.section\b|\.amdhsa_kernel\b)")
    out = {}
    for name in names:
        m = re.search(r"^" + re.escape(name) + r":\s*(;.*)?$", asm_text, re.M)
        lines = []
        for line in asm_text[m.end():].split("\n") if m else []:
            if end.match(line):
                break
            s = line.split(";")[0].strip()
            if not s or s[0] == "." or re.match(r"^\S+:$", s):
                continue
            lines.append(re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", ".L", " ".join(s.split())))
        out[name] = lines
    return out


def against(here, there):
    """[(mangled name, verdict)] for two {name: [instruction lines]}"""
    rows = []
    for name in sorted(set(here) | set(there)):
        if name not in there:
            rows.append((name, "only here"))
        elif name not in here:
            rows.append((name, "only there"))
        elif here[name] == there[name]:
            rows.append((name, "identical"))
        else:
            rows.append((name, "differs (%d → %d lines)" % (len(there[name]), len(here[name]))))
    return rows


def resources(asm_text):
    rows = metadata_kernels(asm_text)
    for r in rows:
        r["instruction_lines"] = instruction_lines(asm_text, r["name"])
    names = demangle([r["name"] for r in rows])
    for r in rows:
        r["kernel"] = names[r["name"]]
    return rows


def device_assembly(source, extra=()):
    from voxelhashing_amd import build as vh_build
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "kernels.s")
        cmd = [vh_build.hipcc()] + vh_build.flags(source) + list(extra) + ["--cuda-device-only", "-S", source, "-o", out]
        subprocess.check_call(cmd)
        with open(out) as f:
            return f.read()


def library_resources(lib):
    """the same table (without instruction lines) from a built library: its device code objects' metadata notes"""
    with open(lib, "rb") as f:
        blob = f.read()
    rows, seen, at = [], set(), 0
    while True:
        at = blob.find(b"amdhsa.kernels", at)
        if at < 0:
            break
        rows += notes_at(blob, at)
        at += 1
    out = []
    for r in rows:
        if r["name"] not in seen:
            seen.add(r["name"])
            out.append(r)
    names = demangle([r["name"] for r in out])
    for r in out:
        r["kernel"] = names[r["name"]]
    return out


# ---- the metadata note of a code object is MessagePack: a small reader for the subset the compiler writes

def _unpack(b, i):
    t = b[i]
    if t <= 0x7f:
        return t, i + 1
    if 0x80 <= t <= 0x8f:
        return _map(b, i + 1, t & 0x0f)
    if 0x90 <= t <= 0x9f:
        return _arr(b, i + 1, t & 0x0f)
    if 0xa0 <= t <= 0xbf:
        n = t & 0x1f
        return b[i + 1:i + 1 + n].decode("utf-8", "replace"), i + 1 + n
    if t == 0xc0:
        return None, i + 1
    if t in (0xc2, 0xc3):
        return t == 0xc3, i + 1
    if t in (0xc4, 0xd9):
        n = b[i + 1]
        v = b[i + 2:i + 2 + n]
        return (v.decode("utf-8", "replace") if t == 0xd9 else bytes(v)), i + 2 + n
    if t in (0xc5, 0xda):
        n = int.from_bytes(b[i + 1:i + 3], "big")
        v = b[i + 3:i + 3 + n]
        return (v.decode("utf-8", "replace") if t == 0xda else bytes(v)), i + 3 + n
    if t in (0xc6, 0xdb):
        n = int.from_bytes(b[i + 1:i + 5], "big")
        v = b[i + 5:i + 5 + n]
        return (v.decode("utf-8", "replace") if t == 0xdb else bytes(v)), i + 5 + n
    if t in (0xcc, 0xcd, 0xce, 0xcf):
        n = 1 << (t - 0xcc)
        return int.from_bytes(b[i + 1:i + 1 + n], "big"), i + 1 + n
    if t in (0xd0, 0xd1, 0xd2, 0xd3):
        n = 1 << (t - 0xd0)
        return int.from_bytes(b[i + 1:i + 1 + n], "big", signed=True), i + 1 + n
    if t == 0xca:
        return 0.0, i + 5
    if t == 0xcb:
        return 0.0, i + 9
    if t == 0xdc:
        return _arr(b, i + 3, int.from_bytes(b[i + 1:i + 3], "big"))
    if t == 0xdd:
        return _arr(b, i + 5, int.from_bytes(b[i + 1:i + 5], "big"))
    if t == 0xde:
        return _map(b, i + 3, int.from_bytes(b[i + 1:i + 3], "big"))
    if t == 0xdf:
        return _map(b, i + 5, int.from_bytes(b[i + 1:i + 5], "big"))
    if t >= 0xe0:
        return t - 256, i + 1
    raise ValueError("metadata note: unexpected MessagePack type 0x%02x" % t)


def _arr(b, i, n):
    out = []
    for _ in range(n):
        v, i = _unpack(b, i)
        out.append(v)
    return out, i


def _map(b, i, n):
    out = {}
    for _ in range(n):
        k, i = _unpack(b, i)
        v, i = _unpack(b, i)
        out[k] = v
    return out, i


def notes_at(blob, at):
    """the kernels array whose key string 'amdhsa.kernels' stands at blob[at:]"""
    try:
        kernels, _ = _unpack(blob, at + len(b"amdhsa.kernels"))
    except (ValueError, IndexError):
        return []
    rows = []
    if not isinstance(kernels, list):
        return rows
    for k in kernels:
        if not isinstance(k, dict) or ".name" not in k:
            continue
        row = {"name": k[".name"]}
        for out, key in FIELDS:
            row[out] = int(k.get(key, 0) or 0)
        rows.append(row)
    return rows


def table(rows):
    head = ("kernel", "VGPRs", "SGPRs", "LDS B", "scratch B", "spills", "instr. lines")
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for r in rows:
        lines.append("| `%s` | %d | %d | %d | %d | %d | %s |" % (
            r["kernel"].split("(")[0], r["vgprs"], r["sgprs"], r["lds_bytes"], r["scratch_bytes"],
            r["vgpr_spills"] + r["sgpr_spills"], r.get("instruction_lines", "-")))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("sources", nargs="*", default=[], help="files under voxelhashing_amd/csrc (default: every .hip file of build.SOURCES)")
    ap.add_argument("--match", default="", help="only kernels whose demangled name contains this text")
    ap.add_argument("--json", default="", help="also write the rows to this file")
    ap.add_argument("--library", default="", help="read a built library's metadata instead of compiling")
    ap.add_argument("--against", default="", metavar="DIR", help="another checkout's csrc: compare every kernel's instruction sequence with it")
    args, extra = ap.parse_known_args()
    rows = []
    if args.library:
        rows = library_resources(args.library)
    else:
        from voxelhashing_amd import build as vh_build
        csrc = os.path.join(ROOT, "voxelhashing_amd", "csrc")
        sources = args.sources or [s for s in vh_build.SOURCES if s.endswith(".hip")]
        texts = [device_assembly(s if os.path.isabs(s) else os.path.join(csrc, s), extra) for s in sources]
        if args.against:
            theirs = args.sources or sorted(f for f in os.listdir(args.against) if f.endswith(".hip"))
            here, there = {}, {}
            for t in texts:
                here.update(instruction_sequences(t))
            for s in theirs:
                there.update(instruction_sequences(device_assembly(os.path.join(args.against, os.path.basename(s)), extra)))
            verdicts = against(here, there)
            names = demangle([n for n, _ in verdicts])
            for n, v in verdicts:
                if args.match in names[n]:
                    print("%-28s %s" % (v, names[n].split("(")[0]))
            print("%d kernels: %d identical" % (len(verdicts), sum(v == "identical" for _, v in verdicts)))
            return
        for t in texts:
            rows += resources(t)
    rows = [r for r in rows if args.match in r["kernel"]]
    print(table(rows))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
