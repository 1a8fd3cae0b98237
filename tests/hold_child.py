"""Child process of tests/test_fallback_gpu.py: the "other user" of the GPU.  Holds 7 of 8 compute units with
mc_test_hold_cu for `seconds` on a queue of its own process (HIP deals one process's streams over a few hardware queues, so a
holder in the tests' own process may share the decoder's queue and the step then simply waits behind it; queues of two
processes are never shared).  Prints "held <n>" once the holders are launched, "started <n>" once they have drained.

  python hold_child.py <tests dir> <repo root> <seconds>"""
import sys
import time

sys.path.insert(0, sys.argv[1])  # tests/
sys.path.insert(0, sys.argv[2])  # repo root
import numpy as np  # noqa: E402
import testkernels  # noqa: E402

import metalchat_amd as mc  # noqa: E402

seconds = float(sys.argv[3])
acc = mc.HardwareAccelerator(path=testkernels.build(), ordinal=0)
# 7 of 8 compute units: what is left holds two, at most three of the 512-thread hand-off workgroups each -- not the 256 of the
# launch (half the chip is not enough: the 256 fit two to a CU on the other half).  The holders end by the clock.
nhold = acc.compute_units() // 8 * 7
release = acc.to_device(np.zeros(1, np.uint32))
started = acc.to_device(np.zeros(2, np.uint32))
mc.KernelTask(acc.load("mc_test_hold_cu"), (nhold * 64, 1, 1), (64, 1, 1), [release, started, np.uint64(int(seconds * 1e8))])()
time.sleep(0.2)
print("held", nhold, flush=True)
acc.wait()
print("started", int(started.download(np.uint32, 1)[0]), flush=True)
