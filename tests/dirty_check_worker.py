"""Child process of tests/test_gpu_dirty_check.py: decodes the batches of an .npz file (arrays fix_<name>, two groups each) through
the C ABI with DecodeMethod 2 and the kernel the environment selects (LNSFAID_ZERO_SHIFT), and writes per batch the decoded bits, the
groups' records and the error counters, plus which kernel the context reported.  With rule "codeword" the context is switched to the
per-codeword stop rule (lnsfaid_kernel4cw.hip) and the per-codeword records are written instead.

usage: dirty_check_worker.py <in.npz> <out.npz> [group|codeword]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_abi as oa  # noqa: E402


def main(src, dst, rule="group"):
    abi = oa.pyabi
    lib = abi.load()
    code = abi.Code50GPON(lib)
    batches = np.load(src)
    dec = abi.Decoder(code, abi.default_cfg(2, 10, lib), device=0, max_groups=2, lib=lib)
    on, zg = dec.zero_shift_groups(12)
    if rule == "codeword":
        dec.set_early_stop(abi.STOP_CODEWORD)
    res = {"static": np.array(dec.static_layers()), "zero_shift": np.array(on), "zg": np.array(zg), "waves": np.array(dec.kernel_waves()),
           "early_stop": np.array(dec.early_stop())}
    for key in batches.files:
        name = key[len("fix_"):]
        fix = np.ascontiguousarray(batches[key])
        out, stats = dec.decode_codewords(fix, 2) if rule == "codeword" else dec.decode(fix, 2)
        res["out_" + name], res["stats_" + name] = out, stats
        res["counters_" + name] = np.array(dec.count_errors(out, None, 2), dtype=np.uint64)
    dec.close()
    np.savez(dst, **res)


if __name__ == "__main__":
    main(*sys.argv[1:4])
