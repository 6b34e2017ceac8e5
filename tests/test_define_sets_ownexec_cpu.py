"""The define sets of the owner-narrowed EXEC switch of the 128-ray walk (csrc/packet_rows_kernel.h, -DMRT_ROWS_OWNEXEC=1) still
compile, alone and beside the pop that fetches first (which keeps the stack's top in one of the scalars the switch could want):
compiled the way test_define_sets_cpu.py compiles its list."""
import pytest

import test_define_sets_cpu as ds

DEFINE_SETS = [["-DMRT_ROWS_OWNEXEC=1"], ["-DMRT_ROWS_OWNEXEC=1", "-DMRT_ROWS_POPFETCH=1"]]


@pytest.mark.parametrize("defines", DEFINE_SETS, ids=lambda d: " ".join(d))
def test_walks_compile_with(defines):
    ds.test_walks_compile_with(defines)
