"""Host tests of ``solver.bind_exports`` and of the eight side modules that bind their exports through it (``rl_env``,
``map_stream``, ``path_plan``, ``per_tree``, ``fleet``, ``dqn_fused``, ``dqn_per_fused``, ``collect``): the refusal of a library
that lacks an export, binding twice, tags that do not stand in for each other, and the signatures themselves -- argument counts
written out, as they were when every module set them by hand."""
import ctypes as C
import importlib
import types

import pytest

solver_mod = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.solver")
MODULES = {name: importlib.import_module("trajtrack_mpcndqn_rlboost_amd." + name)
           for name in ("rl_env", "map_stream", "path_plan", "per_tree", "fleet", "dqn_fused", "dqn_per_fused", "collect")}
# module -> (export tuple, table, a source file its refusal names)
BINDINGS = {"rl_env": ("ENV_EXPORTS", "_ENV_TABLE", "csrc/envgpu.hip"), "map_stream": ("MAP_EXPORTS", "_MAP_TABLE", "csrc/mapgpu.hip"),
            "path_plan": ("PLAN_EXPORTS", "_PLAN_TABLE", "csrc/plangpu.hip"), "per_tree": ("PER_EXPORTS", "_PER_TABLE", "csrc/pergpu.hip"),
            "fleet": ("FLEET_EXPORTS", "_FLEET_TABLE", "csrc/trackgpu.hip"), "dqn_fused": ("DQN_EXPORTS", "_DQN_TABLE", "csrc/dqngpu.hip"),
            "dqn_per_fused": ("DQN_PER_EXPORTS", "_DQN_PER_TABLE", "csrc/dqngpu.hip"),
            "collect": ("COLLECT_EXPORTS", "_COLLECT_TABLE", "csrc/envgpu.hip")}
ARGUMENTS = {
    "mpcgpu_env_record_doubles": 1, "mpcgpu_env_step_dev": 11, "mpcgpu_env_step_autoreset_dev": 15, "mpcgpu_env_last_error": 0,
    "mpcgpu_env_img_state_doubles": 1, "mpcgpu_env_step_imgs_dev": 14, "mpcgpu_env_step_imgs_autoreset_dev": 18,
    "mpcgpu_env_step_fresh_dev": 19, "mpcgpu_env_step_imgs_fresh_dev": 22, "mpcgpu_map_spec_doubles": 0, "mpcgpu_map_draw_dev": 7,
    "mpcgpu_map_rings_dev": 7, "mpcgpu_map_record_dev": 12, "mpcgpu_map_last_error": 0,
    "mpcgpu_plan_record_doubles": 1, "mpcgpu_plan_paths_dev": 10, "mpcgpu_plan_last_error": 0,
    "mpcgpu_per_state_doubles": 0, "mpcgpu_per_reset_dev": 5, "mpcgpu_per_add_dev": 8, "mpcgpu_per_update_dev": 7,
    "mpcgpu_per_sample_dev": 10, "mpcgpu_per_stats_dev": 6, "mpcgpu_per_last_error": 0,
    "mpcgpu_fleet_share_dev": 10, "mpcgpu_tracker_step_rows_dev": 15,
    "mpcgpu_dqn_state_floats": 0, "mpcgpu_dqn_grad_dev": 14, "mpcgpu_dqn_apply_dev": 6, "mpcgpu_dqn_step_dev": 14,
    "mpcgpu_dqn_train_dev": 15, "mpcgpu_dqn_last_error": 0, "mpcgpu_dqn_train_per_dev": 19, "mpcgpu_dqn_per_last_error": 0,
    "mpcgpu_collect_act_dev": 11, "mpcgpu_collect_rays_dev": 26, "mpcgpu_collect_last_error": 0}


def _exports(name):
    return getattr(MODULES[name], BINDINGS[name][0])


@pytest.mark.parametrize("name", sorted(BINDINGS))
def test_export_tuple_is_the_key_tuple_of_the_table(name):
    exports, table = _exports(name), getattr(MODULES[name], BINDINGS[name][1])
    assert isinstance(exports, tuple) and exports == tuple(table)
    assert set(ARGUMENTS) == {e for n in BINDINGS for e in _exports(n)}     # every export of every module is listed above
    assert len(ARGUMENTS) == sum(len(_exports(n)) for n in BINDINGS)        # and no two tables share one
    for export, (restype, argtypes) in table.items():
        assert len(argtypes) == ARGUMENTS[export], export
        assert restype is (C.c_char_p if export.endswith("_last_error") else C.c_int32), export


@pytest.mark.parametrize("name", sorted(BINDINGS))
def test_a_library_that_lacks_an_export_is_refused_by_name(name):
    exports = _exports(name)
    for gone in exports:
        stand_in = types.SimpleNamespace(**{e: types.SimpleNamespace() for e in exports if e != gone})
        with pytest.raises(solver_mod.MpcGpuError) as err:
            MODULES[name]._bind(stand_in)
        text = str(err.value)
        assert gone in text and BINDINGS[name][2] in text and "rebuild" in text and "no fallback" in text
        assert not any(hasattr(fn, "argtypes") for fn in vars(stand_in).values())      # refused before anything was set
    whole = types.SimpleNamespace(**{e: types.SimpleNamespace() for e in exports})
    assert MODULES[name]._bind(whole) is whole
    assert all(len(whole.__dict__[e].argtypes) == ARGUMENTS[e] for e in exports)


def test_binding_twice_keeps_the_handle_and_the_signatures():
    lib = solver_mod.load_library()
    for _ in range(2):
        for name in sorted(BINDINGS):
            assert MODULES[name]._bind(lib) is lib
        for name in sorted(BINDINGS):
            for export in _exports(name):
                fn = getattr(lib, export)
                assert len(fn.argtypes) == ARGUMENTS[export], export
                assert fn.restype is (C.c_char_p if export.endswith("_last_error") else C.c_int32), export


@pytest.mark.parametrize("name", sorted(BINDINGS))
def test_tags_do_not_stand_in_for_each_other(name):
    """The tag is the table's own: a handle bound for every other module's table is still asked for this module's exports."""
    others = [n for n in sorted(BINDINGS) if n != name]
    stand_in = types.SimpleNamespace(**{e: types.SimpleNamespace() for n in others for e in _exports(n)})
    for n in others:
        MODULES[n]._bind(stand_in)
    with pytest.raises(solver_mod.MpcGpuError, match=_exports(name)[0]):
        MODULES[name]._bind(stand_in)
