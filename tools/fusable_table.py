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
import sys
import zlib

F32, BF16 = 0, 1  # include/moegan_hip.h MG_F32 / MG_BF16
# (slot, value) lists; slot numbers: csrc/mg_plan.h
SETTINGS = [[], [(5, 1)], [(3, 64)], [(3, 128)], [(3, 257)], [(2, 64)], [(2, 128)], [(2, 256)], [(2, 257)], [(9, 2)],
            [(11, 1)], [(29, 1)], [(16, 1)], [(16, 2)], [(16, 3)]]
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
    """{setting: packed answers}, every slot restored to 0 afterwards."""
    tab = {}
    for setting in SETTINGS:
        for slot, value in setting:
            lib.mg_set_tuning(slot, value)
        try:
            bits = answers(lib)
        finally:
            for slot, _ in setting:
                lib.mg_set_tuning(slot, 0)
        tab[",".join(f"{s}={v}" for s, v in setting) or "default"] = {"n": len(bits), "ones": sum(bits),
                                                                       "bits": pack(bits)}
    return tab


if __name__ == "__main__":
    with open(sys.argv[2], "w") as f:
        json.dump(table(load(sys.argv[1])), f, indent=1)
        f.write("\n")
