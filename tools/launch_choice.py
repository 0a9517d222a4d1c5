#!/usr/bin/env python3
"""Which kernel runs which stack under which flags: the record of the launch policy (csrc/wbcqp_host_handle.hpp, choose_kernel).

    python tools/launch_choice.py 2> choice.txt

One launch of each shipped stack under each of the handle flags that bear on the choice, plus one ragged launch of two stacks, with
WBCQP_DEBUG_LAUNCH=1: the library's "wbcqp occupancy:" / "wbcqp launch:" lines go to stderr, each launch under a "== stack flags" line of this
script.  Not a test: two builds are compared by comparing what this prints, line for line."""
import os
import sys

os.environ["WBCQP_DEBUG_LAUNCH"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

STACKS = ["talos", "talos_single_support", "icub", "icub_single_support", "franka", "tiago", "three_contact", "talos_torque"]
FLAGS = ["none", "WARM_START", "HW_DISPATCH", "QUEUE", "FULL_LDS", "GENERIC_KERNEL", "WORKGROUP_PER_QP"]
BATCH = 512


def main():
    import torch
    from inria_wbc_amd import capi, structure, synth
    dev = torch.device("cuda", 0)
    sp = torch.cuda.current_stream().cuda_stream

    def arrays(st, seed):
        inputs = synth.generate(st, BATCH, seed)
        d_in = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inputs.items() if v.size}
        out = dict(x=torch.zeros(BATCH, st.n, dtype=torch.float64, device=dev), tau=torch.zeros(BATCH, st.na, dtype=torch.float64, device=dev),
                   status=torch.zeros(BATCH, dtype=torch.int32, device=dev), iters=torch.zeros(BATCH, dtype=torch.int32, device=dev),
                   active_mask=torch.zeros(BATCH, 8, dtype=torch.int32, device=dev))
        return d_in, out

    def say(line):
        sys.stderr.write(line + "\n")
        sys.stderr.flush()

    for name in STACKS:
        st = structure.STRUCTURES[name]()
        d_in, out = arrays(st, 4242)
        for flag in FLAGS:
            say("== %s %s" % (name, flag))
            h = capi.Handle(0, capi.F64, flags=0 if flag == "none" else getattr(capi, "FLAG_" + flag))
            h.set_structure(0, st)
            h.solve_batch(0, BATCH, d_in, out, stream=sp)
            torch.cuda.synchronize()
            h.close()
    say("== ragged talos + icub none")
    sts = [structure.STRUCTURES[n]() for n in ("talos", "icub")]
    h = capi.Handle(0, capi.F64, flags=0)
    groups = []
    for slot, st in enumerate(sts):
        h.set_structure(slot, st)
        d_in, out = arrays(st, 4242 + slot)
        groups.append((slot, BATCH, d_in, out))
    h.solve_ragged(groups, stream=sp)
    torch.cuda.synchronize()
    h.close()


if __name__ == "__main__":
    main()
