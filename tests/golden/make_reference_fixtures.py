#!/usr/bin/env python3
"""Stores the data the tests compare against the reference's own files, so that they run without its tree.

    python tests/golden/make_reference_fixtures.py <root of the VoxelHashing tree>

reference/zParameters*.txt    the reference's three parameter files, byte for byte (tests/test_parameter_file.py,
                              tests/test_camera_tracking.py)
reference/mc_tables.npz       edgeTable[256] and triTable[256][16] of DepthSensingCUDA/Source/Tables.h (Paul Bourke's
                              published marching-cubes tables) as numbers: edge_table int32 [256], tri_table int8
                              [256, 16], -1 where a case has no more edges (tests/test_marching_cubes.py)
"""
import os
import re
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference")
PARAMETER_FILES = ["zParametersDefault.txt", "zParametersManolisScan.txt", "zParametersTrackingDefault.txt"]


def mc_tables(text):
    tri = [int(x) for x in re.findall(r"-?\d+", re.search(r"triTable\[256\]\[16\]\s*=\s*\{(.*?)\};", text, re.S).group(1))]
    edge = [int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]+", re.search(r"edgeTable\[256\]\s*=\s*\{(.*?)\};", text, re.S).group(1))]
    assert len(tri) == 4096 and len(edge) == 256
    return np.array(edge, dtype=np.int32), np.array(tri, dtype=np.int8).reshape(256, 16)


def main(ref_root):
    os.makedirs(OUT, exist_ok=True)
    for name in PARAMETER_FILES:
        shutil.copyfile(os.path.join(ref_root, name), os.path.join(OUT, name))
    edge, tri = mc_tables(open(os.path.join(ref_root, "DepthSensingCUDA", "Source", "Tables.h")).read())
    np.savez_compressed(os.path.join(OUT, "mc_tables.npz"), edge_table=edge, tri_table=tri)
    for name in sorted(os.listdir(OUT)):
        print(name, os.path.getsize(os.path.join(OUT, name)), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
