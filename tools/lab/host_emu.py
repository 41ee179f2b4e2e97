"""Stage a solver library's kernel source for the host emulation of tools/lab/eightpoint_host/shim.h and build it: the one copy of
what every tools/lab/*_host/run.py does before it runs its checks.

Every rel_pose_amd/csrc/*.h is copied into the temporary directory with csrc/common.h replaced by shim.h, the kernel source becomes
kernel.cpp there, and the `../csrc/` and `../../include/` includes of all of them are flattened (the compiler finds the copies and
include/ on its search path).  The harness's main.cpp, which includes kernel.cpp, is then built with g++ under AddressSanitizer and
UBSan into a stand-alone program; nothing is written into the tree."""
import os
import re
import subprocess

LAB = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(LAB))
SHIM = os.path.join(LAB, "eightpoint_host")


def _staged(text):
    text = re.sub(r'#include "(\.\./csrc/)?common\.h"', '#include "shim.h"', text)
    return re.sub(r'#include "(?:\.\./csrc/|\.\./\.\./include/)(\w+\.h)"', r'#include "\1"', text)


def build(source, here, tmp, flags=()):
    """source: the kernel file relative to rel_pose_amd/; here: the harness directory (main.cpp); returns the program's path"""
    pkg = os.path.join(ROOT, "rel_pose_amd")
    for h in sorted(os.listdir(os.path.join(pkg, "csrc"))):
        if h.endswith(".h") and h != "common.h":
            open(os.path.join(tmp, h), "w").write(_staged(open(os.path.join(pkg, "csrc", h)).read()))
    open(os.path.join(tmp, "kernel.cpp"), "w").write(_staged(open(os.path.join(pkg, source)).read()))
    exe = os.path.join(tmp, "emu")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-w", "-fsanitize=address,undefined", *flags, "-I", tmp, "-I", SHIM,
                           "-I", os.path.join(ROOT, "include"), os.path.join(here, "main.cpp"), "-o", exe])
    return exe
