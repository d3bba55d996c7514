"""The eighth list of ABI families of boxinstseg_amd/_lib.py (LEVELSET_FAMILIES: the mask losses of BoxSOLOv2Head.loss, which arrived after
tests/test_abi_families.py pinned FAMILIES, tests/test_abi_family_inst.py pinned LATE_FAMILIES, tests/test_abi_family_dconv16.py pinned
HALF_FAMILIES, tests/test_abi_family_dconvl.py pinned LEVEL_FAMILIES, tests/test_abi_family_rle.py pinned RESULT_FAMILIES,
tests/test_abi_family_b2m.py pinned TRAIN_FAMILIES and tests/test_abi_family_dbx.py pinned PSEUDO_FAMILIES) against its headers, the
library's exports and the guarded GPU tests: the four checks of tests/test_abi_family_dbx.py, for this list.

* what the family's header declares = the keys of its signature table = exported symbols, with the tabled restype / argtypes applied and
  as many parameters as the C declaration has;
* no name shared with any table or header of any family of any of the eight lists; a duplicate fails at load with the unchanged message;
* every entry point is run guarded by a named test of tests/test_gpu_guarded_bls_loss.py (its GUARDED table) or exempt here as a size query.
No GPU needed: only the built library."""
import importlib
import inspect

import pytest

from boxinstseg_amd import _lib
from tests.test_abi_families import _declarations

GUARDED_MODULES = {'bls': ('test_gpu_guarded_bls_loss',)}
# entry point -> why no guarded test runs it: nothing here launches a kernel over caller memory
EXEMPT = {'bxi_bls_state_bytes': 'size query', 'bxi_bls_high_state_bytes': 'size query'}
EARLIER = (_lib.FAMILIES + _lib.LATE_FAMILIES + _lib.HALF_FAMILIES + _lib.LEVEL_FAMILIES + _lib.RESULT_FAMILIES + _lib.TRAIN_FAMILIES
           + _lib.PSEUDO_FAMILIES)
EVERY = EARLIER + _lib.LEVELSET_FAMILIES


@pytest.fixture(scope='module', autouse=True)
def _built(built):
    return built


def test_levelset_families_are_the_bls_table():
    assert [name for name, _, _ in _lib.LEVELSET_FAMILIES] == ['bls'] and _lib.LEVELSET_FAMILIES[0][2] is _lib.BLS_SIGNATURES
    assert _lib.LEVELSET_FAMILIES[0][1] == ('include/boxinst/boxinst_hip_bls.h',)
    assert sorted(_lib.BLS_SIGNATURES) == ['bxi_bls_backward_f32', 'bxi_bls_front_f32', 'bxi_bls_high_backward_f32', 'bxi_bls_high_forward_f32',
                                           'bxi_bls_high_state_bytes', 'bxi_bls_state_bytes']
    assert set(GUARDED_MODULES) == {name for name, _, _ in _lib.LEVELSET_FAMILIES}
    assert len({name for name, _, _ in EVERY}) == len(EVERY)
    assert all(table is not _lib.BLS_SIGNATURES for _, _, table in EARLIER)
    assert [name for name, _, _ in _lib.PSEUDO_FAMILIES] == ['dbx']              # the seventh list stays as it was pinned
    assert _lib.load().bxi_abi_version() == _lib.BXI_ABI_VERSION == 7          # additive: the version stays


def test_constants_agree_with_the_header():
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'boxinst', 'boxinst_hip_bls.h')) as fh:
        code = fh.read()
    define = lambda n: eval(re.search(r'#define\s+' + n + r'\s+(\(?[0-9 <]+\)?)', code).group(1))
    assert define('BXI_BLS_MAX_GROUPS') == _lib.BLS_MAX_GROUPS == _lib.SOLO_MAX_FACTORS
    assert define('BXI_BLS_MAX_LEVELS') == _lib.BLS_MAX_LEVELS == _lib.DET_MAX_LEVELS
    assert define('BXI_BLS_MAX_W') == _lib.BLS_MAX_W and define('BXI_BLS_CHUNK_PIXELS') == _lib.BLS_CHUNK_PIXELS
    assert define('BXI_BLS_LEVEL_ROWS') == _lib.BLS_LEVEL_ROWS


@pytest.mark.parametrize('family,headers,table', _lib.LEVELSET_FAMILIES, ids=[f[0] for f in _lib.LEVELSET_FAMILIES])
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
    for other, other_headers, other_table in EVERY:
        if other != family:
            assert not set(table) & set(other_table), (family, other, sorted(set(table) & set(other_table)))
            again = set(decls) & set(_declarations(other_headers))
            assert not again, f'{sorted(again)} of {family} declared again in {other_headers}'


@pytest.mark.parametrize('family,table', [(f[0], f[2]) for f in _lib.LEVELSET_FAMILIES], ids=[f[0] for f in _lib.LEVELSET_FAMILIES])
def test_a_name_in_two_families_fails_at_load(monkeypatch, family, table):
    name = sorted(table)[0]
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LEVELSET_FAMILIES', _lib.LEVELSET_FAMILIES + [('again', (), {name: table[name]})])
    with pytest.raises(RuntimeError, match=f'{name} is in the signature tables of two ABI families: {family} and again'):
        _lib.load()
    # and across the lists: a name of the first table of each of the seven earlier lists, in this one
    for first_family, _, first_table in (_lib.FAMILIES[0], _lib.LATE_FAMILIES[0], _lib.HALF_FAMILIES[0], _lib.LEVEL_FAMILIES[0], _lib.RESULT_FAMILIES[0],
                                         _lib.TRAIN_FAMILIES[0], _lib.PSEUDO_FAMILIES[0]):
        stolen = sorted(first_table)[0]
        monkeypatch.setattr(_lib, '_lib', None)
        monkeypatch.setattr(_lib, 'LEVELSET_FAMILIES', [('levelset', (), {stolen: first_table[stolen]})])
        with pytest.raises(RuntimeError, match=f'{stolen} is in the signature tables of two ABI families: {first_family} and levelset'):
            _lib.load()


def _guarded(family):
    """entry point -> (module, test) over the family's GUARDED tables: the named test exists and its module makes the call."""
    found = {}
    for mod_name in GUARDED_MODULES[family]:
        mod = importlib.import_module('tests.' + mod_name)
        for entry, test in mod.GUARDED.items():
            assert entry not in found, f'{entry} is listed twice'
            fn = getattr(mod, test, None)
            assert callable(fn) and test.startswith('test_'), f'{entry}: {mod_name} has no test {test}'
            assert '_call(' in inspect.getsource(fn), (entry, test)
            assert 'lib.' + entry + '(' in inspect.getsource(mod._call), entry
            found[entry] = (mod_name, test)
    return found


@pytest.mark.parametrize('family,table', [(f[0], f[2]) for f in _lib.LEVELSET_FAMILIES], ids=[f[0] for f in _lib.LEVELSET_FAMILIES])
def test_every_entry_point_is_guarded_or_exempt(family, table):
    mine = set(_guarded(family))
    exempt = set(EXEMPT) & set(table)
    assert not mine & exempt, sorted(mine & exempt)
    missing = set(table) - mine - exempt
    assert not missing, f'{family}: neither run by a guarded test (GUARDED) nor exempt with a reason (EXEMPT): {sorted(missing)}'
    assert mine | exempt == set(table), f'{family}: not in its signature table any more: {sorted((mine | exempt) - set(table))}'
    for entry, reason in EXEMPT.items():
        assert reason and '_bytes' in entry, entry
