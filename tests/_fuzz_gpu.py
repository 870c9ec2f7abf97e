"""What tests/test_gpu_fuzz_layers.py, tests/test_gpu_fuzz_ops.py and tests/test_gpu_fuzz_detect.py share (a helper module, not a
conftest): the upload, the bit-for-bit comparator, the loop over a chunk's cases and the record of the kernel names each family's
calls left behind.  `cases`: the module that holds the family -- tests/_fuzz_cases.py, or tests/_fuzz_detect_cases.py."""
import numpy as np
import pytest
import torch

from tests import _fuzz_cases as FC
from tests import _interp_ref as IR

SEEN = {}  # family -> {chunk: the kernel names its calls recorded}; one record for both case modules: their family names do not collide


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(got, want, what):
    """Bit for bit but for a NaN's payload (tests/test_gpu_fcos.py::_bits_equal, tests/test_gpu_mask.py::_same_bits)."""
    got, want = got.detach().cpu().contiguous(), torch.from_numpy(np.ascontiguousarray(want))
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, (what, got.shape, want.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN positions differ"
    a, b = IR.bits(got)[~nan], IR.bits(want)[~nan]
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {b.numel()} elements differ"


def sweep(family, chunk, run, with_reference=True, cases=FC):
    """run(case, d, want) every case of a chunk; want is None in a run for the kernel names alone."""
    names = set()
    for case in cases.cases(family, chunk):
        d = cases.inputs(case)
        names.update(run(case, d, cases.reference(case, d) if with_reference else None))
    SEEN.setdefault(family, {})[chunk] = names
    return names


def kernels_of(family, run, cases=FC):
    for chunk in cases.chunks(family):
        if chunk not in SEEN.get(family, {}):
            sweep(family, chunk, run, with_reference=False, cases=cases)
    return set().union(*SEEN[family].values())


def chunked(family, cases=FC):
    return pytest.mark.parametrize("chunk", list(cases.chunks(family)))
