"""Child process of tests/test_gpu_bf_stage.py: decodes the batches of an .npz file (arrays fix_<name>, three groups each, with
iter_<name> = MaxIteration) through the C ABI with DecodeMethod 2 on the kernel the environment selects (LNSFAID_ZERO_SHIFT,
LNSFAID_WAVES_PER_CODEWORD, LNSFAID_MSG_STORE), and writes per batch the decoded bits, the groups' records and the error counters,
plus which kernel the context reported.

usage: bf_stage_worker.py <in.npz> <out.npz>"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_abi as oa  # noqa: E402


def main(src, dst):
    abi = oa.pyabi
    lib = abi.load()
    code = abi.Code50GPON(lib)
    batches = np.load(src)
    res = {}
    for key in batches.files:
        if not key.startswith("fix_"):
            continue
        name = key[len("fix_"):]
        dec = abi.Decoder(code, abi.default_cfg(2, int(batches["iter_" + name]), lib), device=0, max_groups=3, lib=lib)
        on, _ = dec.zero_shift_groups(12)
        res.update({"static": np.array(dec.static_layers()), "zero_shift": np.array(on), "waves": np.array(dec.kernel_waves()),
                    "msg_store": np.array(dec.message_store())})
        out, stats = dec.decode(np.ascontiguousarray(batches[key]), 3)
        res["out_" + name], res["stats_" + name] = out, stats
        res["counters_" + name] = np.array(dec.count_errors(out, None, 3), dtype=np.uint64)
        dec.close()
    np.savez(dst, **res)


if __name__ == "__main__":
    main(*sys.argv[1:3])
