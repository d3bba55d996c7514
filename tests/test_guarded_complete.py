"""Host side of the guarded tests: every entry point of the C ABI is either run guarded by a named test or exempt for a stated reason,
and the helper itself (tests/guarded.py) does what it says.  No GPU needed."""
import inspect

import pytest
import torch

from tests import guarded as G

# entry point -> why no guarded test runs it: nothing here launches a kernel over caller memory
EXEMPT = {
    'bxi_abi_version': 'version query',
    'bxi_status_string': 'status text',
    'bxi_last_hip_error': 'status query',
    'bxi_check_device': 'device query',
    'bxi_dev_set_launch_hook': 'developer hook (bxi_dev_*)',
    'bxi_dev_set_tree_level_walk': 'developer switch (bxi_dev_*)',
    'bxi_dev_sol_eval_f32': 'benchmark-only speed-of-light kernel (bxi_dev_*)',
    'bxi_dev_sol_pairwise_f32': 'benchmark-only speed-of-light kernel (bxi_dev_*)',
    'bxi_boxinst_loss_workspace_bytes': 'size query',
    'bxi_boxinst_loss_state_bytes': 'size query',
    'bxi_boxinst_loss_state_status_offset': 'offset query',
    'bxi_boxinst_loss_state_warmup_offset': 'offset query',
    'bxi_boxinst_eval_workspace_bytes': 'size query',
    'bxi_boxinst_eval_workspace_lab_offset': 'offset query',
    'bxi_dynamic_mask_backward_workspace_bytes': 'size query',
    'bxi_dynamic_mask_generic_backward_workspace_bytes': 'size query',
    'bxi_meanfield_workspace_bytes': 'size query',
    'bxi_mil_loss_state_bytes': 'size query',
    'bxi_levelset_state_bytes': 'size query',
    'bxi_lcm_workspace_bytes': 'size query',
    'bxi_mst_workspace_bytes': 'size query',
    'bxi_bfs_workspace_bytes': 'size query',
    'bxi_tree_refine_workspace_bytes': 'size query',
    'bxi_tree_refine_backward_weight_workspace_bytes': 'size query',
}


def _tables():
    from tests import test_gpu_guarded_abi as abi, test_gpu_guarded_modules as mods
    return {abi: abi.GUARDED, mods: mods.GUARDED}


def test_every_entry_point_is_guarded_or_exempt():
    """A new entry point fails here until somebody decides which of the two it is."""
    from boxinstseg_amd import _lib
    tables = _tables()
    guarded = {}
    for mod, table in tables.items():
        for entry, test in table.items():
            assert entry not in guarded, f'{entry} is listed twice'
            fn = getattr(mod, test, None)
            assert callable(fn), f'{entry}: {mod.__name__} has no test {test}'
            assert entry in inspect.getsource(mod), entry
            guarded[entry] = test
    assert not set(guarded) & set(EXEMPT), sorted(set(guarded) & set(EXEMPT))
    for entry in _lib.SIGNATURES:
        assert entry in guarded or entry in EXEMPT, f'{entry}: neither run by a guarded test (GUARDED) nor exempt with a reason (EXEMPT)'
    stale = (set(guarded) | set(EXEMPT)) - set(_lib.SIGNATURES)
    assert not stale, f'not in _lib.SIGNATURES any more: {sorted(stale)}'
    for entry, reason in EXEMPT.items():
        assert reason and ('_bytes' in entry or '_offset' in entry or entry.startswith('bxi_dev_') or entry in
                           ('bxi_abi_version', 'bxi_status_string', 'bxi_last_hip_error', 'bxi_check_device')), entry


@pytest.mark.parametrize('dtype,lead', [(torch.float32, 0), (torch.float32, 3), (torch.float64, 1), (torch.int32, 1), (torch.int64, 1), (torch.uint8, 15)])
def test_embed_places_the_view_and_the_poison(dtype, lead):
    t = (torch.arange(24) % 7).to(dtype).view(2, 3, 4)
    g = G.embed(t, lead, 128)
    assert g.t.is_contiguous() and g.t.shape == t.shape and g.t.storage_offset() == 128 + lead and torch.equal(g.t, t)
    assert g.backing.numel() == 128 + lead + 24 + 128
    assert (g.ptr() - g.backing.data_ptr()) == (128 + lead) * t.element_size()
    lo, hi = g.backing[:128 + lead], g.backing[128 + lead + 24:]
    if dtype.is_floating_point:
        assert bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())
    elif dtype == torch.uint8:
        assert bool((lo == 255).all()) and bool((hi == 255).all())
    else:
        assert bool((lo == -1).all()) and bool((hi == -1).all())           # -1: range checks reject it, as an offset it stays in the band
    G.check_bands(g)
    G.check_unchanged(g)
    g.t.view(-1)[5] += 1
    with pytest.raises(AssertionError, match='modified'):
        G.check_unchanged(g)
    g.backing[128 + lead - 1] = 0
    with pytest.raises(AssertionError, match='outside'):
        G.check_bands(g)
    with pytest.raises(AssertionError):
        G.embed(t, 16 // t.element_size(), 128)                           # below 16 bytes only
    with pytest.raises(AssertionError):
        G.embed(t, 0, 100)                                                # bands are multiples of 64 elements


def test_outputs_carry_the_pattern_until_written():
    for dtype, bits in ((torch.float32, 0x7FC5A5A5), (torch.int32, 0x5A5A5A5A), (torch.uint8, 0xA5)):
        g = G.out((3, 5), dtype, 'cpu', 1, 64)
        iv = g.backing if dtype != torch.float32 else g.backing.view(torch.int32)
        assert bool((iv == bits).all())
        G.check_bands(g)
        with pytest.raises(AssertionError):
            G.check_written(g)
        g.t.fill_(1)
        G.check_written(g)
        g.t[1, 2] = torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32) if dtype == torch.float32 else bits
        with pytest.raises(AssertionError):
            G.check_written(g)                                             # one element left (a 0xA5 byte is not a 0 / 1 mask value)
        g.t.fill_(0)
        g.backing[g.start + g.numel] = 0
        with pytest.raises(AssertionError, match='band after'):
            G.check_bands(g)
    assert G.plane_band(24, 40, 4) == 1216 and G.plane_band(4, 4) == 1024 and G.plane_band(336, 304, 2) % 64 == 0


def test_poisoned_empty_patches_and_restores():
    real = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    base = torch.zeros(4)
    with G.poisoned_empty():
        a, b, c = torch.empty(5), torch.empty_like(base), base.new_empty((2, 2), dtype=torch.int32)
        d, e = torch.empty((3,), dtype=torch.uint8), torch.empty(0)
        assert bool((a.view(torch.int32) == G.PATTERN_F32).all()) and bool((b.view(torch.int32) == G.PATTERN_F32).all())
        assert bool((c == 0x5A5A5A5A).all()) and bool((d == 0xA5).all()) and e.numel() == 0
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real
    with pytest.raises(ZeroDivisionError):
        with G.poisoned_empty():
            1 / 0
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real
