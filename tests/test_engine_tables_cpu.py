"""CPU: the tables the engine classes are built from, held against the ctypes signature table (_lib.SIGNATURES = every
symbol include/rgp.h declares).  No device, no library.

The models and stream.py probe engines with hasattr / getattr (forward_rows, status, persistent, bptt_persistent,
backward_stream), so which members a class has is behaviour: a class exposes a member exactly when its family's C ABI has
the entry behind it.  Two exceptions are part of the contract and are pinned here as they are:
  FcGruEngine / buffer_elems   the ABI has the entry, the engine's read_buffer goes by its own table of shapes (BUFFER_SHAPES)
  Grcn77Engine / inject_fault  the ABI has no entry, the member exists to refuse by name (NotImplementedError)."""
import pytest

from recurrent_gaze_prediction_amd import _lib, engine as E

# class name -> (C prefix, create entry behind it, weights struct)
FAMILIES = {
    'GrcnEngine': ('rgp_grcn_', 'create', _lib.GrcnWeights),
    'C3dConvEngine': ('rgp_c3dconv_', 'create', _lib.C3dConvWeights),
    'LstmEngine': ('rgp_lstm_', 'create', _lib.LstmWeights),
    'Grcn77Engine': ('rgp_grcn77_', 'create', _lib.Grcn77Weights),
    'FcGruEngine': ('rgp_fcgru_', 'create_flags', _lib.FcGruWeights),
    'ShallowNetEngine': ('rgp_shallownet_', 'create_ex', _lib.ShallowNetWeights),
    'CascadeEngine': ('rgp_cascade_', 'create_ex', _lib.CascadeWeights),
    'C3DEngine': ('rgp_c3d_', 'create_ex', _lib.C3DWeights),
    'ActionEngine': ('rgp_action_', 'create', _lib.ActionWeights),
}
# entry behind the prefix -> the member of the class that stands on it
OPTIONAL = {'status': 'status', 'state_elems': 'state_elems', 'persistent_workgroups': 'persistent_workgroups',
            'bptt_persistent_workgroups': 'bptt_persistent_workgroups', 'inject_fault': 'inject_fault',
            'buffer_elems': 'read_buffer_elems', 'forward_rows': 'forward_rows', 'backward_input': 'backward_input',
            'backward_stream': 'backward_stream'}
ABI_ONLY = {('FcGruEngine', 'buffer_elems')}
REFUSES = {('Grcn77Engine', 'inject_fault')}
NAMES = sorted(FAMILIES)


@pytest.mark.parametrize('name', NAMES)
def test_the_entries_every_plan_owner_resolves_exist(name):
    cls = getattr(E, name)
    prefix, create, weights = FAMILIES[name]
    for attr, want in (('PREFIX', prefix), ('CREATE', create), ('WEIGHTS', weights)):
        if getattr(cls, attr, None) is not None:            # a class that declares it declares this
            assert getattr(cls, attr) == want, (name, attr)
    for entry in (create, 'destroy', 'workspace_bytes', 'bind_workspace', 'set_weights'):
        assert prefix + entry in _lib.SIGNATURES, (name, entry)


@pytest.mark.parametrize('name', NAMES)
def test_every_optional_entry_has_its_member_and_no_member_stands_on_nothing(name):
    cls = getattr(E, name)
    prefix = FAMILIES[name][0]
    for entry, member in OPTIONAL.items():
        in_abi, exposed = prefix + entry in _lib.SIGNATURES, hasattr(cls, member)
        if (name, entry) in ABI_ONLY:
            assert in_abi and not exposed, (name, entry)
        elif (name, entry) in REFUSES:
            assert exposed and not in_abi, (name, entry)
            with pytest.raises(NotImplementedError):
                getattr(cls, member)(object.__new__(cls))
        else:
            assert in_abi == exposed, (name, entry, in_abi, exposed)
    # the members that go with one of the above
    assert hasattr(cls, 'persistent') == hasattr(cls, 'persistent_workgroups')
    assert hasattr(cls, 'bptt_persistent') == hasattr(cls, 'bptt_persistent_workgroups')
    assert hasattr(cls, 'forward_stream') == hasattr(cls, 'state_elems') == (prefix + 'forward_stream' in _lib.SIGNATURES)
    assert hasattr(cls, 'read_buffer') == (prefix + 'read_buffer' in _lib.SIGNATURES)


def test_the_absences_the_models_rely_on():
    assert not hasattr(E.FcGruEngine, 'forward_rows') and not hasattr(E.FcGruEngine, 'backward_input')
    assert not hasattr(E.C3dConvEngine, 'status') and not hasattr(E.C3dConvEngine, 'persistent')
    assert not hasattr(E.CascadeEngine, 'status') and not hasattr(E.ShallowNetEngine, 'state_elems')
    assert [n for n in NAMES if hasattr(getattr(E, n), 'backward_stream')] == ['FcGruEngine', 'GrcnEngine']


@pytest.mark.parametrize('name', NAMES)
def test_every_parameter_maps_to_a_field_of_the_weights_struct(name):
    cls = getattr(E, name)
    weights = FAMILIES[name][2]
    if name == 'C3DEngine':                                  # two arrays of eight pointers, laid out by rgp_c3d_param_offset
        assert [f for f, _ in weights._fields_] == ['w', 'b'] and len(E.C3D_LAYER_NAMES) == 8
        return
    fields = set(weights.FIELDS)
    table = getattr(cls, 'PARAM_TO_FIELD', None)             # None: every field under its own name
    if table is not None:
        assert set(table.values()) <= fields and len(set(table.values())) == len(table), name
    assert set(getattr(cls, 'UNTRAINED', ())) <= set(table or fields)
    if name == 'ActionEngine':
        for mode, t in E.ACTION_PARAM_TO_FIELD.items():
            assert set(t.values()) <= fields, mode
            assert [f for f in weights.FIELDS if f in t.values()] == list(t.values()), mode     # the struct's order
    if name == 'CascadeEngine':
        assert tuple(f for f, _ in cls.KEYS) == tuple(weights.FIELDS)
    if name in ('GrcnEngine', 'C3dConvEngine', 'LstmEngine', 'Grcn77Engine'):
        assert list(table.values()) == list(weights.FIELDS), name                               # the flat buffer's order


def test_grad_groups_are_contiguous_runs_of_the_parameter_list():
    names = list(E.GRCN_PARAM_TO_FIELD)
    runs = []
    for group, first, last in E.GrcnEngine.GRAD_GROUPS:
        lo, hi = names.index(first), names.index(last)
        assert lo <= hi, (first, last)
        runs.append((lo, hi))
    assert [g for g, _, _ in E.GrcnEngine.GRAD_GROUPS] == [_lib.RGP_GRCN_GRADS_TOP, _lib.RGP_GRCN_GRADS_GRU, _lib.RGP_GRCN_GRADS_PROJ]
    # completion order is back to front, and together the runs are the whole list, each variable once
    assert runs == sorted(runs, reverse=True)
    covered = sorted(i for lo, hi in runs for i in range(lo, hi + 1))
    assert covered == list(range(len(names)))
