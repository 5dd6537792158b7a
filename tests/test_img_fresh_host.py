"""Host-side tests (no GPU) of the fresh-map image step of ``include/mpcgpu_map.h``: the export, its argument binding and its
refusals before anything is enqueued."""
import ctypes
import importlib
import os

from trajtrack_mpcndqn_rlboost_amd import map_stream, rl_env

solver_mod = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.solver")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "mpcgpu_env_step_imgs_fresh_dev"


def _lib():
    return rl_env._bind(map_stream._bind(solver_mod.load_library()))


def _params(n_edge_max=40):
    return rl_env._CParams(num_segments=8, corner_samples=3, n_path_max=8, n_obst_max=2, n_kf_max=2, n_edge_max=n_edge_max,
                           time_step=0.2, **rl_env.ROBOT)


def test_the_library_exports_the_entry_and_only_the_map_header_declares_it():
    assert ENTRY in map_stream.MAP_EXPORTS and ENTRY not in rl_env.ENV_EXPORTS
    lib = ctypes.CDLL(solver_mod.library_path())
    assert hasattr(lib, ENTRY)
    assert ENTRY + "(" in open(os.path.join(ROOT, "include", "mpcgpu_map.h")).read()
    assert ENTRY not in open(os.path.join(ROOT, "include", "mpcgpu_env.h")).read()
    lib.mpcgpu_abi_version.restype = ctypes.c_int32
    assert lib.mpcgpu_abi_version() == 8                     # a new entry in a side header: the version stays


def test_null_tables_are_refused_without_a_device():
    lib = _lib()
    params, img = _params(), rl_env.image_params()
    entry = getattr(lib, ENTRY)
    assert len(entry.argtypes) == 4 + 16 + 2
    assert entry(0, ctypes.byref(params), ctypes.byref(img), 4, *([None] * 16), 10, None) < 0
    assert b"null pointer" in lib.mpcgpu_env_last_error()


def test_refusals_before_anything_is_enqueued():
    """Host buffers stand in for the device pointers: every call below must return before it touches one of them."""
    lib = _lib()
    entry = getattr(lib, ENTRY)
    params, img = _params(), rl_env.image_params()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    # order: records2, which, spare_ready, loaded, stale, state, img_state, distance_field, action, obs_internal, obs_image,
    #        reward, terminated, truncated, terminal_obs_internal, terminal_obs_image
    full = [p] * 16

    def call(ptrs, max_steps=10, par=params, im=img, B=4):
        rc = entry(0, ctypes.byref(par), ctypes.byref(im), B, *ptrs, max_steps, None)
        return rc, lib.mpcgpu_env_last_error().decode()

    for i in (1, 2, 3, 4, 6, 7, 10):                         # which, spare_ready, loaded, stale, img_state, distance_field, obs_image
        rc, text = call([None if j == i else p for j in range(16)])
        assert rc < 0 and "null pointer" in text, (i, text)
    rc, text = call(full, max_steps=-1)
    assert rc < 0 and "negative" in text
    rc, text = call([None if j == 8 else p for j in range(16)])          # auto-reset without actions
    assert rc < 0 and "actions" in text
    rc, text = call([None if j == 13 else p for j in range(16)])         # auto-reset without truncated
    assert rc < 0 and "truncated" in text
    rc, text = call(full, im=rl_env.image_params(width=4))
    assert rc < 0 and "mpcgpu_env_img_params" in text
    rc, text = call(full, par=_params(n_edge_max=1100))      # 2 * 1100 * 24 bytes of edge staging + 17 KB > 64 KB
    assert rc < 0 and "too many outline edges" in text
