"""Stage the reference's voxel-hashing sources for a host build (oracle/ref/Makefile).

    python oracle/ref/stage.py REFERENCE_ROOT OUT_DIR
    python oracle/ref/stage.py --list REFERENCE_ROOT      (the files it reads, for the Makefile's dependencies)

Copies the files listed in FILES from the reference tree into OUT_DIR (oracle/_ref/src, never committed) and makes
the mechanical edits a host C++ compiler needs.  Every edit is a rule about syntax; this script holds no text of the
reference:

  * a kernel launch `k<<<grid, block>>>(args);` becomes `vhr_launch(grid, block, k, args);`, the launch emulator of
    oracle/ref/include/cuda_runtime.h;
  * `__align__(n) struct Name` becomes `struct __align__(n) Name`: the stand-in spells __align__ as a GNU attribute,
    which applies to the type only after the class key (nvcc's spelling is MSVC's __declspec, which goes before it);
  * an out-of-class definition of a member of an explicit class-template specialisation (`inline ... X<3, 1>::...`)
    gets the `template<>` that nvcc lets it omit and clang does not;
  * in the two files of _CONST_REF_FILES only (the RGB-D build unit and the matrix header it uses), a matrix parameter
    `matNxM<..>& NAME` / `mat1x6& NAME` whose NAME is in _READ_ONLY_REF_PARAMS becomes a const reference: the host
    compiler the reference was built with (MSVC) binds a temporary to a non-const reference, the tracker's kernel
    passes products of matrices to such parameters, and the functions only read them.

The reference's own mLib.h is not copied: a quoted include searches the including file's directory first, so a copy
next to the sources would win over the stand-in in oracle/ref/include.
"""
import os
import re
import shutil
import sys

# (directory relative to the reference root, file name)
FILES = [("DepthSensingCUDA/Source", n) for n in (
    "VoxelUtilHashSDF.h", "RayCastSDFUtil.h", "DepthCameraUtil.h", "CUDAHashParams.h", "CUDARayCastParams.h",
    "CUDADepthCameraParams.h", "cuda_SimpleMatrixUtil.h", "cudaUtil.h",
    "CUDASceneRepHashSDF.cu", "CUDARayCastSDF.cu", "CameraUtil.cu", "CUDASceneRepChunkGrid.cu",
    "CUDAMarchingCubesSDF.cu", "MarchingCubesSDFUtil.h", "Tables.h",
    "CUDAImageHelper.cu", "CUDABuildLinearSystem.cu", "CUDABuildLinearSystemRGBD.cu", "ICPUtil.h",
    "CameraTrackingInput.h")] + [
    ("DepthSensingCUDA/Include/cutil/inc", "cutil_math.h")]

# `name <<< a, b >>> ( args ) ;` -- nvcc accepts blanks between the angle brackets, so the tokens are matched one by one
_LAUNCH = re.compile(r"(\w+)\s*<\s*<\s*<(?P<cfg>[^;]*?)>\s*>\s*>\s*\((?P<args>.*?)\)\s*;", re.S)
# `inline ... Name<int, int>::member` at the start of a line: an explicit specialisation's member defined out of class
_SPEC_MEMBER = re.compile(r"^\s*inline\b[^;{(]*\w+\s*<\s*\d+\s*(,\s*\d+\s*)*>\s*::")


# `__align__(n)` (and comments or blanks) directly before `struct Name`
_ALIGN_STRUCT = re.compile(r"__align__\((\d+)\)(?P<gap>(\s|//[^\n]*)*)struct\s+(?P<name>\w+)")


# reference parameters that receive temporaries and are only read (setBlock's source, addToLocalSystem's two rows)
_CONST_REF_FILES = ("cuda_SimpleMatrixUtil.h", "CUDABuildLinearSystemRGBD.cu")
_READ_ONLY_REF_PARAMS = ("input", "jacobianBlockRow", "residualsBlockRow")
_REF_PARAM = re.compile(r"(?<!const )\b(mat\w+(?:<[^<>]*>)?)&\s*(%s)\b" % "|".join(_READ_ONLY_REF_PARAMS))


def _split_top(s):
    """split s at the commas outside parentheses"""
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    out.append(cur)
    return [p.strip() for p in out]


def _launch(m):
    cfg = _split_top(m.group("cfg"))
    if len(cfg) > 2 and cfg[2] not in ("0",):
        raise SystemExit(f"stage.py: launch of {m.group(1)} asks for dynamic shared memory or a stream: {cfg}")
    args = m.group("args").strip()
    return f"vhr_launch(dim3({cfg[0]}), dim3({cfg[1]}), {m.group(1)}{', ' + args if args else ''});"


def edit(text, name=""):
    text = _LAUNCH.sub(_launch, text)
    text = _ALIGN_STRUCT.sub(lambda m: f"{m.group('gap')}struct __align__({m.group(1)}) {m.group('name')}", text)
    if name in _CONST_REF_FILES:
        text = _REF_PARAM.sub(r"const \1& \2", text)
    lines = text.split("\n")
    out = []
    for ln in lines:
        if _SPEC_MEMBER.match(ln):
            prev = next((p for p in reversed(out) if p.strip()), "")
            if not prev.strip().startswith("template"):
                out.append("template<>")
        out.append(ln)
    return "\n".join(out)


def main(ref_root, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for sub, name in FILES:
        src = os.path.join(ref_root, sub, name)
        with open(src, "r", encoding="latin-1") as f:
            text = f.read()
        dst = os.path.join(out_dir, name)
        tmp = dst + ".tmp"
        with open(tmp, "w", encoding="latin-1") as f:
            f.write(edit(text, name))
        os.replace(tmp, dst)
    # a stale copy of a file dropped from FILES must not linger
    keep = {n for _, n in FILES}
    for n in os.listdir(out_dir):
        if n not in keep:
            p = os.path.join(out_dir, n)
            shutil.rmtree(p) if os.path.isdir(p) else os.remove(p)


if __name__ == "__main__":
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    if sys.argv[1] == "--list":
        print(" ".join(os.path.join(sys.argv[2], sub, name) for sub, name in FILES))
    else:
        main(sys.argv[1], sys.argv[2])
