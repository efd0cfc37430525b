"""The stand-alone host programs of the sweep's device-free headers (tests/sweep_plan_host.cpp, sweep_pack_host.cpp,
sweep_blocks_host.cpp): one way to build them, plain and under ASan and UBSan.  Each has its own main and is run directly."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_FLAGS = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def build_host_program(tmp_path_factory, source, flags):
    """tests/<source> compiled with HOST_FLAGS + flags into a directory of its own; returns the program's path"""
    name = os.path.splitext(source)[0] + ("_san" if flags else "")
    out = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++"] + HOST_FLAGS + flags + [os.path.join(HERE, source), "-o", out])
    return out
