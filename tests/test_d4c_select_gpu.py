"""D4C's band selection alone on the MI355X (include/world_hip.h: world_hip_probe_select): the cases of
test_d4c_select_cpu.py through the shipped library -- the GPU's own v_readlane / ballot / DPP spellings of the select's wave
collectives on every route, where the analysis tests meet only the routes their data happens to take -- then the Python layer."""
import numpy as np
import pytest

import test_d4c_select_cpu as cpu
from backends import OnGpu, gpu_backend, wh  # noqa: F401 (wh: a fixture)

pytestmark = pytest.mark.gpu


class GpuBackend(OnGpu, cpu.Backend):
    pass


be = gpu_backend(GpuBackend)


# ---- the cases of the CPU file -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", cpu.NTS)
def test_every_route_and_every_entry_of_the_general_routine(be, nt):
    cpu.case_routes(be, nt)


@pytest.mark.parametrize("nt", cpu.NTS)
def test_inside_the_general_routine(be, nt):
    cpu.case_general(be, nt)


@pytest.mark.parametrize("nt", cpu.NTS)
def test_where_the_threshold_and_the_top_key_live(be, nt):
    cpu.case_positions(be, nt)


@pytest.mark.parametrize("nt", cpu.NTS)
def test_every_served_k(be, nt):
    cpu.case_every_k(be, nt)


@pytest.mark.parametrize("nt", cpu.NTS)
def test_real_valued_rows_within_the_any_order_bound(be, nt):
    cpu.case_real(be, nt)


@pytest.mark.parametrize("nt", cpu.NTS)
def test_a_row_depends_on_nothing_but_the_row(be, nt):
    cpu.case_rows_are_independent(be, nt)


def test_refusals_write_nothing_and_name_the_argument(be):
    cpu.case_refusals(be)


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_probe_select_of_the_python_layer(wh, be):
    import torch
    nt = 256
    batch = cpu.batches_routes(nt)[0]
    keys, want = cpu.lattice_reference(batch, "2^-80")
    d = torch.from_numpy(np.array(keys)).cuda()                         # (a copy: the shared reference is read-only)
    for mode in (0, 1):
        out = wh.probe_select(d, batch.K, mode=mode).cpu().numpy()
        assert out.shape == (len(keys), 3) and cpu.same_bits(out, be.run(mode, keys, batch.K))
        assert cpu.same_bits(out[:, :2], want) and np.array_equal(out[:, 2], batch.routes if mode == 0 else np.full(len(keys), 2.0))
    with pytest.raises(RuntimeError, match="K"):
        wh.probe_select(d, 0)
    with pytest.raises(RuntimeError, match="threads"):
        wh.probe_select(d[:, :100].contiguous(), 5)
