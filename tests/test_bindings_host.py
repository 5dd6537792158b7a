"""Host tests of ``solver.bind_exports``, of the eight side modules that bind their exports through it (``rl_env``,
``map_stream``, ``path_plan``, ``per_tree``, ``fleet``, ``dqn_fused``, ``dqn_per_fused``, ``collect``) and of the core library's
own table (``solver.load_library``): the refusal of a library that lacks an export, binding twice, tags that do not stand in
for each other, and the signatures themselves -- argument counts written out, as they were when every module set them by
hand."""
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
    "mpcgpu_collect_act_dev": 11, "mpcgpu_collect_rays_dev": 26, "mpcgpu_collect_last_error": 0,
    # the core library (include/mpcgpu.h) and the two exports of its trace build
    "mpcgpu_abi_version": 0, "mpcgpu_create": 2, "mpcgpu_destroy": 1, "mpcgpu_last_error": 1, "mpcgpu_num_params": 1,
    "mpcgpu_solve_batch": 15, "mpcgpu_solve_batch_dev": 16, "mpcgpu_cost_grad_batch": 10, "mpcgpu_psi_value_batch": 6,
    "mpcgpu_last_timing": 3, "mpcgpu_last_eval_counts": 5, "mpcgpu_last_shape": 5, "mpcgpu_last_waves_per_simd": 1,
    "mpcgpu_reserve_shape": 5, "mpcgpu_set_option": 3, "mpcgpu_last_problems_per_wavefront": 1, "mpcgpu_last_ordered": 1,
    "mpcgpu_last_tail_promotion": 3, "mpcgpu_last_tail_timeouts": 3, "mpcgpu_last_tail_timing": 3, "mpcgpu_last_latency_kernel": 1,
    "mpcgpu_reserve_batch": 2, "mpcgpu_last_table_kind": 1, "mpcgpu_tracker_window_dev": 4, "mpcgpu_tracker_step_dev": 11,
    "mpcgpu_rl_reference_dev": 11, "mpcgpu_hint_switch_dev": 19, "mpcgpu_debug_read_workspace": 3, "mpcgpu_workspace_stride": 1,
    "mpcgpu_workspace_record": 1, "mpcgpu_debug_prep": 3, "mpcgpu_debug_tracker_assemble": 3, "mpcgpu_debug_lbfgs_direction": 8,
    "mpcgpu_debug_set_trace": 2, "mpcgpu_debug_read_trace": 3}
# the core exports a library may lack: the first four in an older build loaded for an A/B run, the last two outside the trace build
CORE_OPTIONAL = ("mpcgpu_psi_value_batch", "mpcgpu_last_tail_promotion", "mpcgpu_last_tail_timeouts", "mpcgpu_last_tail_timing")
TRACE = ("mpcgpu_debug_set_trace", "mpcgpu_debug_read_trace")


def _exports(name):
    return getattr(MODULES[name], BINDINGS[name][0])


@pytest.mark.parametrize("name", sorted(BINDINGS))
def test_export_tuple_is_the_key_tuple_of_the_table(name):
    exports, table = _exports(name), getattr(MODULES[name], BINDINGS[name][1])
    assert isinstance(exports, tuple) and exports == tuple(table)
    core = solver_mod.EXPORTS + TRACE
    assert set(ARGUMENTS) == {e for n in BINDINGS for e in _exports(n)} | set(core)     # every export of every table is listed above
    assert len(ARGUMENTS) == sum(len(_exports(n)) for n in BINDINGS) + len(core)        # and no two tables share one
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


def _core_restype(export):
    return None if export == "mpcgpu_destroy" else C.c_char_p if export == "mpcgpu_last_error" else C.c_int32


def test_core_table_lists_every_export_with_its_argument_count():
    table = solver_mod._CORE_TABLE
    assert isinstance(solver_mod.EXPORTS, tuple) and solver_mod.EXPORTS == tuple(table) and len(table) == 33
    assert tuple(solver_mod._TRACE_TABLE) == TRACE and not set(TRACE) & set(table)
    assert set(solver_mod._CORE_OPTIONAL) == set(CORE_OPTIONAL) < set(table)
    for export, (restype, argtypes) in {**table, **solver_mod._TRACE_TABLE}.items():
        assert len(argtypes) == ARGUMENTS[export], export
        assert restype is _core_restype(export), export
    lib = solver_mod.load_library()
    for export in solver_mod.EXPORTS:
        fn = getattr(lib, export)
        assert len(fn.argtypes) == ARGUMENTS[export] and fn.restype is _core_restype(export), export
    assert not any(hasattr(lib, export) for export in TRACE)               # the product library is no trace build


def test_a_library_that_lacks_a_mandatory_core_export_is_refused_by_name():
    exports = solver_mod.EXPORTS
    for gone in exports:
        if gone in CORE_OPTIONAL:
            continue
        stand_in = types.SimpleNamespace(**{e: types.SimpleNamespace() for e in exports if e != gone})
        with pytest.raises(solver_mod.MpcGpuError) as err:
            solver_mod._bind(stand_in)
        text = str(err.value)
        assert gone in text and "csrc/mpcgpu.hip" in text and "rebuild" in text and "no fallback" in text
        assert not any(e in text for e in exports if e != gone and not gone.startswith(e))
        assert not any(hasattr(fn, "argtypes") for fn in vars(stand_in).values())      # refused before anything was set


def test_a_library_that_lacks_only_the_optional_core_exports_is_accepted():
    exports = solver_mod.EXPORTS
    for absent in (CORE_OPTIONAL, CORE_OPTIONAL[:1], CORE_OPTIONAL[1:], ()):
        for trace in (False, True):
            names = [e for e in exports if e not in absent] + (list(TRACE) if trace else [])
            stand_in = types.SimpleNamespace(**{e: types.SimpleNamespace() for e in names})
            assert solver_mod._bind(stand_in) is stand_in
            assert all(len(stand_in.__dict__[e].argtypes) == ARGUMENTS[e] for e in names)
            assert all(stand_in.__dict__[e].restype is _core_restype(e) for e in names if e not in TRACE)
            assert not any(hasattr(stand_in, e) for e in absent) and hasattr(stand_in, TRACE[0]) == trace


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
