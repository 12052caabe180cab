"""The library's pure-host "is this call covered" answers over a fixed grid, as packed bits per tuning setting.

mg_modconv_dgrad_fusable, mg_conv2d_wgrad_bias_fusable and mg_gemm_wgrad_bias_fusable touch no device, so the shared
object is loaded with ctypes and no GPU is needed.  tests/test_fusable_table_cpu.py evaluates the same grid on the
built library and requires equality with tests/fusable_table.json, which was written by

    python tools/fusable_table.py <libmoegan_hip.so of the commit before the dispatch plans> tests/fusable_table.json

The file pins the answers the hand-kept copies of the dispatch rules gave; it is not regenerated from later code.
"""
import base64
import ctypes
import itertools
import json
import os
import re
import sys
import zlib

F32, BF16 = 0, 1  # include/moegan_hip.h MG_F32 / MG_BF16
# slot name -> number: the MG_TUNE_* table of include/moegan_hip.h (read as moegan_mi/_lib.py reads it)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "moegan_hip.h")
TUNE = {n: int(v) for n, v in re.findall(r"\bMG_TUNE_(\w+)\s*=\s*(\d+)\s*,", open(HEADER).read())}
# (slot, value) lists
SETTINGS = [[], [("NO_SLABS", 1)], [("GEMM_TILE", 64)], [("GEMM_TILE", 128)], [("GEMM_TILE", 257)], [("CONV_TILE", 64)],
            [("CONV_TILE", 128)], [("CONV_TILE", 256)], [("CONV_TILE", 257)], [("SHORTK", 2)], [("DETERMINISTIC", 1)],
            [("MODGRAD_UNFUSED", 1)], [("NARROW", 1)], [("NARROW", 2)], [("NARROW", 3)]]
DTYPES = [BF16, F32]
KS = [1, 3]
BS = [1, 3, 16, 256]
MAPS = [(4, 4), (4, 5), (8, 8), (16, 16), (32, 32), (64, 64)]
CGS = [8, 32, 64, 128, 512]
CINS = [8, 24, 32, 128, 512]
PTR = 0x10000  # a 16-byte aligned address; the queries never dereference it


def load(path):
    lib = ctypes.CDLL(path)
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    lib.mg_set_tuning.argtypes = [i, i]
    lib.mg_get_tuning.argtypes = [i]
    lib.mg_modconv_dgrad_fusable.argtypes = [i] * 8 + [p, i64, p, i64, p, i64]
    lib.mg_conv2d_wgrad_bias_fusable.argtypes = [i, i, i, i, p, i, i, i, i, i]
    lib.mg_gemm_wgrad_bias_fusable.argtypes = [i]
    return lib


def answers(lib):
    """One 0 / 1 per grid point, in a fixed order."""
    out = []
    for dt, gdt, k, B, (H, W), Cg, Cin, mis in itertools.product(DTYPES, DTYPES, KS, BS, MAPS, CGS, CINS, (0, 1)):
        out.append(lib.mg_modconv_dgrad_fusable(dt, gdt, k, B, H, W, Cg, Cin, PTR, 3 * Cin + 8, PTR, Cin + 4 * mis,
                                                PTR + 8 * mis, Cin))
    for dt, (H, W), Cin, Cout, k, sc in itertools.product(DTYPES, MAPS, CINS, CGS, KS, (0, 1)):
        out.append(lib.mg_conv2d_wgrad_bias_fusable(dt, H, W, Cin, PTR if sc else None, Cout, k, k, 1, k // 2))
    out += [lib.mg_gemm_wgrad_bias_fusable(dt) for dt in DTYPES]
    assert all(v in (0, 1) for v in out)
    return out


def pack(bits):
    n = int("".join(map(str, bits)), 2)
    return base64.b64encode(zlib.compress(n.to_bytes((len(bits) + 7) // 8, "big"), 9)).decode()


def table(lib):
    """{setting (the numeric slot=value spec): packed answers}, every slot restored to what it held."""
    tab = {}
    for setting in SETTINGS:
        held = [(TUNE[name], lib.mg_get_tuning(TUNE[name])) for name, _ in setting]
        for name, value in setting:
            lib.mg_set_tuning(TUNE[name], value)
        try:
            bits = answers(lib)
        finally:
            for slot, old in reversed(held):
                lib.mg_set_tuning(slot, old)
        tab[",".join(f"{TUNE[n]}={v}" for n, v in setting) or "default"] = {"n": len(bits), "ones": sum(bits),
                                                                           "bits": pack(bits)}
    return tab


if __name__ == "__main__":
    with open(sys.argv[2], "w") as f:
        json.dump(table(load(sys.argv[1])), f, indent=1)
        f.write("\n")
