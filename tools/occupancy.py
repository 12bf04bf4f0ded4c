#!/usr/bin/env python3
"""Resident workgroups per CU of the metric topology's step kernels, as the HIP runtime computes them from the kernel's registers
and the dynamic LDS the library asks for (hipOccupancyMaxActiveBlocksPerMultiprocessor):  occupancy.py [lib.so]
The kernel handles are the library's exported symbols; the LDS bytes come from truss_topo_lds_info."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mop-truss-marl_amd"), ROOT]
import numpy as np
import torch
import truss_mi355 as tm
from truss_mi355 import synthetic

lib = tm.load(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else None)
assert lib.backend == "hip" and torch.cuda.is_available()
torch.zeros(1, device="cuda")                       # the HIP runtime is up
hip = C.CDLL("libamdhip64.so")
topo = synthetic.bench_topology(16, 4)
h = topo.native(lib)
KERNELS = (("step<16,8,1,5>", "_Z17truss_step_kernelILi16ELi8ELi1ELi5ELb0EEv7TopoDev11StepArgsDev", 0, 64),
           ("rollout<16,8,1,5>", "_Z20truss_rollout_kernelILi16ELi8ELi1ELi5EEv10RolloutDev", 0, 64),
           ("step<16,8,1,5,EMIT>", "_Z17truss_step_kernelILi16ELi8ELi1ELi5ELb1EEv7TopoDev11StepArgsDev", 1, 128))
for name, sym, emit, threads in KERNELS:
    info = np.zeros(16, np.int32)
    lib.check(lib.dll.truss_topo_lds_info(h, emit, info.ctypes.data_as(C.c_void_p), None, 0, None, 0), "truss_topo_lds_info")
    f = C.c_void_p.in_dll(lib.dll, sym)             # the kernel's handle: what hipLaunchKernel is given
    rc = hip.hipFuncSetAttribute(C.byref(f), 8, 160 * 1024)      # hipFuncAttributeMaxDynamicSharedMemorySize
    n = C.c_int(-1)
    rc2 = hip.hipOccupancyMaxActiveBlocksPerMultiprocessor(C.byref(n), C.byref(f), threads, C.c_size_t(int(info[0])))
    print(f"{name:22s} LDS/workgroup {int(info[0]):6d} B  threads {threads:3d}  resident workgroups per CU {n.value}  (rc {rc} {rc2})")
