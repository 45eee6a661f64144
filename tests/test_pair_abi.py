"""The opt-in register-resident kernel for any three-layer bank (gmx_pair.hip), as far as a machine without a GPU
can check it: which topologies gmx_topology_register_rows_eligible accepts, and that none of the kernel's
instantiations spills (its record loads are issued by hand: a spill of one of their destinations would be stored
before the data is in)."""
import os
import re
import subprocess

import pytest

from gmix_amd import bank, topology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def three(n, l0, l1, skip=(1,), final=True):
    return topology.Topology(n, [(0, 8, .01)] * l0 + [(1, 5, .01)] * l1 + ([(2, 3, .01)] if final else []), skip=skip)


ELIGIBLE = {
    "stock90": lambda: topology.stock(90),
    "256x24/8/1": lambda: topology.synth3(256),
    "91x24/8/1": lambda: three(91, 24, 8),
    "40x5/3/1": lambda: three(40, 5, 3),
    "4x1/1/1": lambda: three(4, 1, 1),
    "skip at n-1": lambda: three(200, 24, 8, skip=(199,)),
}
NOT_ELIGIBLE = {
    "l0=25": lambda: three(90, 25, 8),
    "l1=9": lambda: three(90, 24, 9),
    "two skip inputs": lambda: three(90, 24, 8, skip=(1, 2)),
    "no skip input": lambda: three(90, 24, 8, skip=()),
    "no final mixer": lambda: three(90, 24, 8, final=False),
    "no layer 1": lambda: three(90, 24, 0),
    "n=257": lambda: three(257, 24, 8),
    "n=3": lambda: three(3, 2, 2),
    "a single mixer": lambda: topology.single(64, 256, 0.005),
}


@pytest.mark.parametrize("name", list(ELIGIBLE))
def test_eligible(name):
    assert bank.register_rows_eligible(ELIGIBLE[name]()) is True


@pytest.mark.parametrize("name", list(NOT_ELIGIBLE))
def test_not_eligible(name):
    assert bank.register_rows_eligible(NOT_ELIGIBLE[name]()) is False


def test_invalid_topology_is_an_error():
    with pytest.raises(bank.GmxError) as e:
        bank.register_rows_eligible(topology.Topology(16, [(0, 8, .1), (2, 1, .1), (2, 1, .1)]))   # two finals
    assert e.value.status == -1


def test_pair_kernel_does_not_spill():
    src = os.path.join(ROOT, "gmix_amd", "csrc")
    out = subprocess.run(
        ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
         "-fno-gpu-flush-denormals-to-zero", "-c", os.path.join(src, "gmx_pair.hip"), "-o", "/dev/null",
         "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=src)
    report = out.stderr + out.stdout
    blocks = re.split(r"Function Name: ", report)[1:]
    kernels = {}
    for blk in blocks:
        name = re.search(r"gmx_pair_kernelILi(\d+)ELb([01])", blk)
        if not name:
            continue
        kernels[(int(name.group(1)), int(name.group(2)))] = tuple(
            int(re.search(pat + r": (\d+)", blk).group(1))
            for pat in (r" VGPRs", r"AGPRs", r"ScratchSize \[bytes/lane\]", r"VGPRs Spill"))
    assert sorted(kernels) == [(h, m) for h in (32, 64, 96, 144) for m in (0, 1)], (sorted(kernels), report[-2000:])
    msg = {k: dict(zip(("vgprs", "agprs", "scratch", "vgpr_spill"), v)) for k, v in kernels.items()}
    for k, (_v, _a, scratch, spill) in kernels.items():
        assert scratch == 0 and spill == 0, msg
