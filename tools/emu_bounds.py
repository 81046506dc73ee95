"""Builds and runs tools/emu_bounds/main.cpp: the kernel sources on the CPU emulation under AddressSanitizer + UBSan, every buffer a heap
block of exactly its tensor or queried size (see the head of main.cpp).  A stand-alone CPU program; never part of pytest.

    python tools/emu_bounds.py [--no-ubsan] [--record FILE]

The emulation is one translation unit that takes minutes to compile with the sanitizers: its object file is cached under
tools/emu_bounds/build/ on a hash of its sources and flags, and only main.cpp is compiled again when the list of calls changes.
--record appends the command line, every call with the kernels it reached, and "clean" or the sanitizer's report to FILE."""
import argparse
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "emu_bounds")
BUILD = os.path.join(SRC, "build")
EMU = os.path.join(ROOT, "tests", "emu")


def emulation_sources():
    srcs = [os.path.join(EMU, "emu_api.cpp"), os.path.join(EMU, "hipemu.h"), os.path.join(ROOT, "include", "mfn_hip.h")]
    for d, _, files in os.walk(os.path.join(ROOT, "maskflownet_amd", "csrc")):
        srcs += [os.path.join(d, f) for f in files if f.endswith((".h", ".inc"))]
    return sorted(srcs)


def build(ubsan=True):
    san = "-fsanitize=address,undefined" if ubsan else "-fsanitize=address"
    flags = ["-O1", "-g1", "-std=c++20", "-pthread", "-DMFN_EMU", "-I", EMU, "-Wno-unused-but-set-variable", san, "-fno-omit-frame-pointer"]
    h = hashlib.sha256(" ".join(flags[:5] + flags[7:]).encode())
    for s in emulation_sources():
        h.update(os.path.relpath(s, ROOT).encode())
        with open(s, "rb") as f:
            h.update(f.read())
    os.makedirs(BUILD, exist_ok=True)
    obj = os.path.join(BUILD, "emu_api_%s.o" % h.hexdigest()[:16])
    if not os.path.exists(obj):
        print("compiling the emulation with %s (minutes) ..." % san, flush=True)
        subprocess.check_call(["g++"] + flags + ["-c", os.path.join(EMU, "emu_api.cpp"), "-o", obj + ".tmp"])
        os.replace(obj + ".tmp", obj)
    exe = os.path.join(BUILD, "emu_bounds")
    subprocess.check_call(["g++"] + flags + [os.path.join(SRC, "main.cpp"), obj, "-o", exe])
    return exe, san


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--no-ubsan", action="store_true", help="AddressSanitizer alone (a quicker build)")
    ap.add_argument("--record", help="append what ran and what it reported to this file")
    args = ap.parse_args()
    exe, san = build(not args.no_ubsan)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    sys.stdout.write(run.stdout)
    sys.stderr.write(run.stderr)
    clean = run.returncode == 0 and not run.stderr.strip()
    verdict = "clean" if clean else "NOT clean (exit status %d)" % run.returncode
    print(verdict)
    if args.record:
        with open(args.record, "a") as f:
            f.write("== sanitized stand-alone run of the emulation (CPU) ==\n$ python tools/emu_bounds.py%s\n(%s; every buffer a heap block of its exact size)\n"
                    % (" --no-ubsan" if args.no_ubsan else "", san))
            f.write(run.stdout)
            if run.stderr.strip():
                f.write("---- report ----\n" + run.stderr)
            f.write(verdict + "\n\n")
    return 0 if clean else 1


if __name__ == "__main__":
    sys.exit(main())
