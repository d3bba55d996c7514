"""Every ABI family of boxinstseg_amd/_lib.py (FAMILIES) against its headers, the library's exports and the guarded GPU tests.

* what the family's header(s) declare = the keys of its signature table = exported symbols, with the tabled restype / argtypes applied
  and as many parameters as the C declaration has; no name in two families' tables or declared by two families' headers;
* every entry point is run guarded by a named test of the family's test_gpu_guarded_* module(s) or exempt here for a stated reason.
No GPU needed: only the built library."""
import functools
import importlib
import inspect
import os
import re

import pytest

from boxinstseg_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# family -> the modules whose GUARDED tables (entry point -> test name) cover it
GUARDED_MODULES = {
    'base': ('test_gpu_guarded_abi', 'test_gpu_guarded_modules'),
    'post': ('test_gpu_guarded_post',),
    'assign': ('test_gpu_guarded_box_match',),
    'det': ('test_gpu_guarded_det',),
    'fcos': ('test_gpu_guarded_box_head_loss',),
    'solo': ('test_gpu_guarded_solo_targets',),
    'corr': ('test_gpu_guarded_corr',),
    'roi': ('test_gpu_guarded_roi',),
    'msda': ('test_gpu_guarded_msda',),
    'seg': ('test_gpu_guarded_seg',),
    'dconv': ('test_gpu_guarded_solo_conv',),
    'attn': ('test_gpu_guarded_attn',),
}
# these two reach the library through the Python surface: the entry point is named in the module, not in the test that runs it
THROUGH_PYTHON = ('test_gpu_guarded_abi', 'test_gpu_guarded_modules')
# module -> its module-level helper that makes every library call: `lib.<entry>(` stands in the helper, `<helper>(` in the named test
THROUGH_HELPER = {'test_gpu_guarded_seg': '_call', 'test_gpu_guarded_solo_conv': '_call'}

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
    'bxi_matrix_nms_workspace_bytes': 'size query',
    'bxi_box_match_workspace_bytes': 'size query',
    'bxi_det_candidates_workspace_bytes': 'size query',
    'bxi_box_nms_workspace_bytes': 'size query',
    'bxi_fcos_workspace_bytes': 'size query',
    'bxi_solo_cate_workspace_bytes': 'size query',
    'bxi_corr_workspace_bytes': 'size query',
    'bxi_roi_feat_norm_workspace_bytes': 'size query',
    'bxi_msda_backward_workspace_bytes': 'size query',
    'bxi_seg_paste_workspace_bytes': 'size query',
    'bxi_solo_dconv_forward_workspace_bytes': 'size query',
    'bxi_solo_dconv_backward_workspace_bytes': 'size query',
    'bxi_masked_attn_forward_workspace_bytes': 'size query',
    'bxi_masked_attn_backward_workspace_bytes': 'size query',
}


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


@functools.lru_cache(maxsize=None)
def _declarations(headers):
    """name -> parameter list of every function the headers declare (comments stripped; the hook typedef is no function)."""
    decls = {}
    for rel in headers:
        with open(os.path.join(ROOT, rel)) as fh:
            code = re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)
        for name in set(re.findall(r'\b(bxi_[a-z0-9_]+)\s*\(', code)) - {'bxi_launch_hook'}:
            assert name not in decls, f'{name} is declared twice'
            found = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', code)
            assert found, f'{name}: no declaration ending in ");" in {rel}'
            decls[name] = [a for a in found.group(1).split(',') if a.strip() and a.strip() != 'void']
    return decls


def test_families_are_every_table_in_order():
    tables = (_lib.SIGNATURES, _lib.POST_SIGNATURES, _lib.ASSIGN_SIGNATURES, _lib.DET_SIGNATURES, _lib.FCOS_SIGNATURES, _lib.SOLO_SIGNATURES,
              _lib.CORR_SIGNATURES, _lib.ROI_SIGNATURES, _lib.MSDA_SIGNATURES, _lib.SEG_SIGNATURES, _lib.DCONV_SIGNATURES, _lib.ATTN_SIGNATURES)
    assert [name for name, _, _ in _lib.FAMILIES] == ['base', 'post', 'assign', 'det', 'fcos', 'solo', 'corr', 'roi', 'msda', 'seg', 'dconv', 'attn']
    assert len(_lib.FAMILIES) == len(tables) and all(table is own for (_, _, table), own in zip(_lib.FAMILIES, tables))
    assert set(GUARDED_MODULES) == {name for name, _, _ in _lib.FAMILIES}
    assert _lib.load().bxi_abi_version() == _lib.BXI_ABI_VERSION == 7          # every family so far was additive: the version stays


@pytest.mark.parametrize('family,headers,table', _lib.FAMILIES, ids=[f[0] for f in _lib.FAMILIES])
def test_header_exports_and_signatures_agree(family, headers, table):
    lib = _lib.load()
    decls = _declarations(headers)
    assert decls, 'no declarations found'
    for n in decls:
        assert hasattr(lib, n), f'{n} declared in {headers} but not exported'
        assert n in table, f'{n} has no ctypes signature in the {family} table'
    assert sorted(table) == sorted(decls)
    for n, (res, args) in table.items():
        fn = getattr(lib, n)
        assert fn.restype == res and list(fn.argtypes) == list(args), n
        assert len(decls[n]) == len(args), f'{n}: {len(decls[n])} parameters declared, {len(args)} tabled'
    for other, other_headers, other_table in _lib.FAMILIES:
        if other != family:
            assert not set(table) & set(other_table), (family, other, sorted(set(table) & set(other_table)))
            again = set(decls) & set(_declarations(other_headers))
            assert not again, f'{sorted(again)} of {family} declared again in {other_headers}'


@pytest.mark.parametrize('family,table', [(f[0], f[2]) for f in _lib.FAMILIES], ids=[f[0] for f in _lib.FAMILIES])
def test_a_name_in_two_families_fails_at_load(monkeypatch, family, table):
    name = sorted(table)[0]
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'FAMILIES', _lib.FAMILIES + [('again', (), {name: table[name]})])
    with pytest.raises(RuntimeError, match=f'{name} is in the signature tables of two ABI families: {family} and again'):
        _lib.load()


def _guarded(family):
    """entry point -> (module, test) over the family's GUARDED tables, each entry held against the source of the test it names."""
    found = {}
    for mod_name in GUARDED_MODULES[family]:
        mod = importlib.import_module('tests.' + mod_name)
        for entry, test in mod.GUARDED.items():
            assert entry not in found, f'{entry} is listed twice'
            fn = getattr(mod, test, None)
            assert callable(fn), f'{entry}: {mod_name} has no test {test}'
            helper = THROUGH_HELPER.get(mod_name)
            if helper:
                assert 'lib.' + entry + '(' in inspect.getsource(getattr(mod, helper)) and helper + '(' in inspect.getsource(fn), entry
            else:
                assert entry in inspect.getsource(mod if mod_name in THROUGH_PYTHON else fn), entry
            found[entry] = (mod_name, test)
    return found


@pytest.mark.parametrize('family,table', [(f[0], f[2]) for f in _lib.FAMILIES], ids=[f[0] for f in _lib.FAMILIES])
def test_every_entry_point_is_guarded_or_exempt(family, table):
    """A new entry point fails here until somebody decides which of the two it is."""
    mine = set(_guarded(family))
    exempt = set(EXEMPT) & set(table)
    assert not mine & exempt, sorted(mine & exempt)
    missing = set(table) - mine - exempt
    assert not missing, f'{family}: neither run by a guarded test (GUARDED) nor exempt with a reason (EXEMPT): {sorted(missing)}'
    assert mine | exempt == set(table), f'{family}: not in its signature table any more: {sorted((mine | exempt) - set(table))}'


def test_guarded_and_exempt_cover_every_entry_point_once():
    guarded = {}
    for family, _, _ in _lib.FAMILIES:
        for entry in _guarded(family):
            assert entry not in guarded, f'{entry} is listed twice: {guarded[entry]} and {family}'
            guarded[entry] = family
    everything = set().union(*(table for _, _, table in _lib.FAMILIES))
    assert not set(guarded) & set(EXEMPT), sorted(set(guarded) & set(EXEMPT))
    assert set(guarded) | set(EXEMPT) == everything, sorted((set(guarded) | set(EXEMPT)) ^ everything)
    for entry, reason in EXEMPT.items():
        assert reason and ('_bytes' in entry or '_offset' in entry or entry.startswith('bxi_dev_') or entry in
                           ('bxi_abi_version', 'bxi_status_string', 'bxi_last_hip_error', 'bxi_check_device')), entry
