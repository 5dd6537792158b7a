"""The refusals of the side modules' C-ABI entries that come before the first HIP call: one case per ``return fail(...)`` in front
of ``hipSetDevice`` in csrc/envgpu.hip, envimg.hip, pergpu.hip, plangpu.hip, mapgpu.hip and dqngpu.hip, each through every entry
that reaches it.  ``tests/golden/make_abi_refusals_fixture.py`` records (entry, case, return code, text of the module's
``*_last_error``) into ``tests/golden/abi_refusals.json``; ``tests/test_abi_refusals_host.py`` replays them.

No device is needed and none is touched: a refused call reads none of its pointers, so every pointer is the address ``P`` or
NULL.  Left out on purpose: everything behind ``hipSetDevice`` (its text names the machine's devices), which includes every
pointer check of pergpu.hip, and mapgpu.hip's "record header larger than the kernel stages", which no params that pass
``layout`` can reach (HEAD_CAP is the header at P = 64, M = 31, K = 4)."""
import ctypes as C
import importlib
import json
import os

from trajtrack_mpcndqn_rlboost_amd import collect, dqn_fused, dqn_per_fused, map_stream, path_plan, per_tree, rl_env

solver_mod = importlib.import_module("trajtrack_mpcndqn_rlboost_amd.solver")
FIXTURE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "abi_refusals.json")
P = 4096                   # any non-null address
NAN, INF = float("nan"), float("inf")
# slot -> its *_last_error export
SLOTS = {"env": "mpcgpu_env_last_error", "collect": "mpcgpu_collect_last_error", "per": "mpcgpu_per_last_error",
         "plan": "mpcgpu_plan_last_error", "map": "mpcgpu_map_last_error", "dqn": "mpcgpu_dqn_last_error",
         "dqn_per": "mpcgpu_dqn_per_last_error"}


def library():
    lib = solver_mod.load_library()
    for mod in (rl_env, collect, map_stream, path_plan, per_tree, dqn_fused, dqn_per_fused):
        mod._bind(lib)
    return lib


def env_params(**kw):
    base = dict(n_path_max=4, n_obst_max=2, n_kf_max=2, n_edge_max=16, num_segments=8, corner_samples=3, time_step=0.2,
                sample_offset=0.0, collision_factor=4.0, reach_goal_factor=3.0, cross_track_factor=0.05,
                excessive_speed_factor=4.0, reference_speed=1.2, path_progress_factor=2.0, **rl_env.ROBOT)
    base.update(kw)
    return rl_env._CParams(**base)


def img_params(**kw):
    base = dict(width=54, height=54, down_sample=2, reserved=0, scale_x=10.0, scale_y=10.0, center_x=0.0, center_y=0.0, angle=0.0)
    base.update(kw)
    return rl_env._CImgParams(**base)


def collect_params(T=4, capacity=64, pos0=0, eps=None):
    p = collect._CCollectParams(seed=1, serial0=0, capacity=capacity, pos0=pos0, T=T)
    for t, e in enumerate([0.5] * 64 if eps is None else eps):
        p.eps[t] = e
    return p


def per_params(**kw):
    base = dict(capacity=64, update_max_freq=100, alpha=0.6, beta=0.4, epsilon=1e-6, initial_priority=1.0)
    base.update(kw)
    return per_tree._CPerParams(**base)


def dqn_params(**kw):
    base = dict(lr=1e-3, gamma=0.99, max_grad_norm=10.0, beta1=0.9, beta2=0.999, eps=1e-8, double_q=1, reserved=0)
    base.update(kw)
    return dqn_fused._CDqnParams(**base)


def plan_params(**kw):
    base = dict(n_vert_max=64, n_ring_max=8, n_node_max=16, reserved=0)
    base.update(kw)
    return path_plan._CPlanParams(**base)


def _ref(struct):
    return None if struct is None else C.byref(struct)


BAD_ENV = {"null": None, "P65": env_params(n_path_max=65), "P1": env_params(n_path_max=1), "M32": env_params(n_obst_max=32),
           "M-1": env_params(n_obst_max=-1), "K0": env_params(n_kf_max=0), "K5": env_params(n_kf_max=5), "E0": env_params(n_edge_max=0)}
UNBUILT_ENV = {"segments16": env_params(num_segments=16), "corners2": env_params(corner_samples=2)}
BAD_IMG = {"null": None, "down_sample4": img_params(down_sample=4), "width7": img_params(width=7), "width97": img_params(width=97),
           "height7": img_params(height=7), "height97": img_params(height=97), "scale_x_nan": img_params(scale_x=NAN),
           "scale_y_inf": img_params(scale_y=INF), "center_x_inf": img_params(center_x=-INF), "center_y_nan": img_params(center_y=NAN),
           "angle_nan": img_params(angle=NAN)}
BAD_PER = {"null": None, "capacity0": per_params(capacity=0), "capacity2^30+1": per_params(capacity=2 ** 30 + 1),
           "freq0": per_params(update_max_freq=0), "alpha<0": per_params(alpha=-0.1), "alpha_nan": per_params(alpha=NAN),
           "beta<0": per_params(beta=-0.1), "beta_inf": per_params(beta=INF), "epsilon<0": per_params(epsilon=-1e-9),
           "priority0": per_params(initial_priority=0.0)}
BAD_DQN = {"null": None, "lr0": dqn_params(lr=0.0), "lr_nan": dqn_params(lr=NAN), "norm0": dqn_params(max_grad_norm=0.0),
           "beta1=1": dqn_params(beta1=1.0), "beta1<0": dqn_params(beta1=-0.1), "beta2=1": dqn_params(beta2=1.0),
           "eps0": dqn_params(eps=0.0), "double_q2": dqn_params(double_q=2)}
BAD_PLAN = {"null": None, "vert2": plan_params(n_vert_max=2), "vert257": plan_params(n_vert_max=257), "ring0": plan_params(n_ring_max=0),
            "ring33": plan_params(n_ring_max=33), "node1": plan_params(n_node_max=1), "node65": plan_params(n_node_max=65)}


def cases(lib):
    """[(entry, case, slot, call)]: ``call()`` is refused and leaves its words in ``slot``."""
    out = []

    def add(entry, slot, case, *args):
        fn = getattr(lib, entry)
        out.append((entry, case, slot, lambda: fn(*args)))

    def named(names, **null):        # P for every name, NULL for those in `null`
        return {k: (None if k in null else P) for k in names}

    # ---- envgpu.hip: the ray entries ----------------------------------------------------------------------------------------
    for case, bad in BAD_ENV.items():
        add("mpcgpu_env_record_doubles", "env", "params " + case, _ref(bad))

    def step(params=env_params(), B=8, **null):
        a = named(["records", "state", "action", "obs_int", "obs_ext", "reward", "terminated"], **null)
        return (0, _ref(params), B, a["records"], a["state"], a["action"], a["obs_int"], a["obs_ext"], a["reward"], a["terminated"], None)

    def autoreset(params=env_params(), B=8, max_steps=3, **null):
        a = named(["records", "state", "action", "obs_int", "obs_ext", "reward", "terminated", "truncated", "term_int", "term_ext"], **null)
        return (0, _ref(params), B, a["records"], a["state"], a["action"], a["obs_int"], a["obs_ext"], a["reward"], a["terminated"],
                a["truncated"], a["term_int"], a["term_ext"], max_steps, None)

    def fresh(params=env_params(), B=8, max_steps=3, **null):
        a = named(["records", "which", "spare_ready", "loaded", "stale", "state", "action", "obs_int", "obs_ext", "reward", "terminated",
                   "truncated", "term_int", "term_ext"], **null)
        return (0, _ref(params), B, a["records"], a["which"], a["spare_ready"], a["loaded"], a["stale"], a["state"], a["action"],
                a["obs_int"], a["obs_ext"], a["reward"], a["terminated"], a["truncated"], a["term_int"], a["term_ext"], max_steps, None)

    for entry, build in (("mpcgpu_env_step_dev", step), ("mpcgpu_env_step_autoreset_dev", autoreset), ("mpcgpu_env_step_fresh_dev", fresh)):
        for case, bad in {**BAD_ENV, **UNBUILT_ENV}.items():
            add(entry, "env", "params " + case, *build(params=bad))
        add(entry, "env", "B -1", *build(B=-1))
        for k in ("records", "state", "obs_int", "obs_ext"):
            add(entry, "env", "null " + k, *build(**{k: True}))
    add("mpcgpu_env_step_autoreset_dev", "env", "null action", *autoreset(action=True))
    for m in (0, -5):
        add("mpcgpu_env_step_autoreset_dev", "env", f"max_steps {m}", *autoreset(max_steps=m))
    for k in ("which", "spare_ready", "loaded", "stale"):
        add("mpcgpu_env_step_fresh_dev", "env", "null " + k, *fresh(**{k: True}))
    add("mpcgpu_env_step_fresh_dev", "env", "max_steps -1", *fresh(max_steps=-1))
    add("mpcgpu_env_step_fresh_dev", "env", "null action", *fresh(action=True))
    add("mpcgpu_env_step_fresh_dev", "env", "null truncated", *fresh(truncated=True))
    add("mpcgpu_env_step_fresh_dev", "env", "null which, max_steps -1", *fresh(which=True, max_steps=-1))      # the order of the checks
    add("mpcgpu_env_step_fresh_dev", "env", "null action and truncated", *fresh(action=True, truncated=True))
    add("mpcgpu_env_step_fresh_dev", "env", "null truncated, params null", *fresh(truncated=True, params=None))

    # ---- envimg.hip ------------------------------------------------------------------------------------------------------------
    for case, bad in BAD_IMG.items():
        add("mpcgpu_env_img_state_doubles", "env", "img " + case, _ref(bad))

    def imgs(params=env_params(), img=img_params(), B=8, **null):
        a = named(["records", "state", "img_state", "dfield", "action", "obs_int", "obs_image", "reward", "terminated"], **null)
        return (0, _ref(params), _ref(img), B, a["records"], a["state"], a["img_state"], a["dfield"], a["action"], a["obs_int"],
                a["obs_image"], a["reward"], a["terminated"], None)

    def imgs_autoreset(params=env_params(), img=img_params(), B=8, max_steps=3, **null):
        a = named(["records", "state", "img_state", "dfield", "action", "obs_int", "obs_image", "reward", "terminated", "truncated",
                   "term_int", "term_image"], **null)
        return (0, _ref(params), _ref(img), B, a["records"], a["state"], a["img_state"], a["dfield"], a["action"], a["obs_int"],
                a["obs_image"], a["reward"], a["terminated"], a["truncated"], a["term_int"], a["term_image"], max_steps, None)

    def imgs_fresh(params=env_params(), img=img_params(), B=8, max_steps=3, **null):
        a = named(["records", "which", "spare_ready", "loaded", "stale", "state", "img_state", "dfield", "action", "obs_int", "obs_image",
                   "reward", "terminated", "truncated", "term_int", "term_image"], **null)
        return (0, _ref(params), _ref(img), B, a["records"], a["which"], a["spare_ready"], a["loaded"], a["stale"], a["state"],
                a["img_state"], a["dfield"], a["action"], a["obs_int"], a["obs_image"], a["reward"], a["terminated"], a["truncated"],
                a["term_int"], a["term_image"], max_steps, None)

    for entry, build in (("mpcgpu_env_step_imgs_dev", imgs), ("mpcgpu_env_step_imgs_autoreset_dev", imgs_autoreset),
                         ("mpcgpu_env_step_imgs_fresh_dev", imgs_fresh)):
        for case, bad in BAD_IMG.items():
            add(entry, "env", "img " + case, *build(img=bad))
        for case, bad in {**BAD_ENV, **UNBUILT_ENV}.items():
            add(entry, "env", "params " + case, *build(params=bad))
        add(entry, "env", "img null, params null", *build(img=None, params=None))
        add(entry, "env", "E 2048: LDS", *build(params=env_params(n_edge_max=2048)))
        add(entry, "env", "B -1", *build(B=-1))
        for k in ("img_state", "dfield", "obs_image", "records", "state", "obs_int"):
            add(entry, "env", "null " + k, *build(**{k: True}))
    add("mpcgpu_env_step_imgs_autoreset_dev", "env", "null action", *imgs_autoreset(action=True))
    for m in (0, -5):
        add("mpcgpu_env_step_imgs_autoreset_dev", "env", f"max_steps {m}", *imgs_autoreset(max_steps=m))
    add("mpcgpu_env_step_imgs_autoreset_dev", "env", "null img_state, img null", *imgs_autoreset(img_state=True, img=None))
    for k in ("which", "spare_ready", "loaded", "stale"):
        add("mpcgpu_env_step_imgs_fresh_dev", "env", "null " + k, *imgs_fresh(**{k: True}))
    add("mpcgpu_env_step_imgs_fresh_dev", "env", "max_steps -1", *imgs_fresh(max_steps=-1))
    add("mpcgpu_env_step_imgs_fresh_dev", "env", "null action", *imgs_fresh(action=True))
    add("mpcgpu_env_step_imgs_fresh_dev", "env", "null truncated", *imgs_fresh(truncated=True))
    add("mpcgpu_env_step_imgs_fresh_dev", "env", "null stale and img_state", *imgs_fresh(stale=True, img_state=True))   # the order of the checks
    add("mpcgpu_env_step_imgs_fresh_dev", "env", "null dfield, max_steps -1", *imgs_fresh(dfield=True, max_steps=-1))
    add("mpcgpu_env_step_imgs_fresh_dev", "env", "null truncated, img null", *imgs_fresh(truncated=True, img=None))

    # ---- envgpu.hip: collection (include/mpcgpu_collect.h) -------------------------------------------------------------------------
    def act(B=8, eps=0.5, **null):
        a = named(["theta", "obs_ext", "obs_int", "actions"], **null)
        return (0, a["theta"], a["obs_ext"], a["obs_int"], B, eps, 1, 0, a["actions"], None, None)

    for k in ("theta", "obs_ext", "obs_int", "actions"):
        add("mpcgpu_collect_act_dev", "collect", "null " + k, *act(**{k: True}))
    add("mpcgpu_collect_act_dev", "collect", "B -1", *act(B=-1))
    for e in (NAN, -0.1, 1.5, INF):
        add("mpcgpu_collect_act_dev", "collect", f"eps {e}", *act(eps=e))
    env_ptrs = ["records", "state", "obs_int", "obs_ext", "reward", "terminated", "truncated", "term_int", "term_ext"]
    ring_ptrs = ["theta", "buf_obs", "buf_next_obs", "buf_actions", "buf_rewards", "buf_dones", "ep_return"]

    def rays(params=env_params(), B=8, max_steps=3, cp=collect_params(), **null):
        a = named(env_ptrs + ring_ptrs, **null)
        return (0, _ref(params), B, *(a[k] for k in env_ptrs), max_steps, a["theta"], _ref(cp), *(a[k] for k in ring_ptrs[1:]),
                None, None, None, None, None)

    for case, bad in {**BAD_ENV, **UNBUILT_ENV}.items():
        add("mpcgpu_collect_rays_dev", "collect", "params " + case, *rays(params=bad))
    for k in env_ptrs + ring_ptrs:
        add("mpcgpu_collect_rays_dev", "collect", "null " + k, *rays(**{k: True}))
    for case, kw in {"null collect": dict(cp=None), "B -1": dict(B=-1), "max_steps 0": dict(max_steps=0), "max_steps -5": dict(max_steps=-5),
                     "T 0": dict(cp=collect_params(T=0)), "T 65": dict(cp=collect_params(T=65, capacity=10 ** 6)),
                     "T -1": dict(cp=collect_params(T=-1)), "capacity 0": dict(cp=collect_params(capacity=0)),
                     "pos0 64": dict(cp=collect_params(pos0=64)), "pos0 -1": dict(cp=collect_params(pos0=-1)),
                     "T * B 32 > 31": dict(cp=collect_params(T=4, capacity=31)), "T * B 512 > 511": dict(cp=collect_params(T=64, capacity=511)),
                     "eps[3] > 1": dict(cp=collect_params(eps=[0.5, 0.5, 0.5, 1.0 + 2.0 ** -52])),
                     "eps[1] < 0": dict(cp=collect_params(eps=[0.5, -1e-300, 0.5, 0.5])),
                     "eps[0] nan": dict(cp=collect_params(eps=[NAN, 0.5, 0.5, 0.5])),
                     "B -1, T 0": dict(B=-1, cp=collect_params(T=0))}.items():
        add("mpcgpu_collect_rays_dev", "collect", case, *rays(**kw))

    # ---- pergpu.hip: the params only (every pointer check stands behind hipSetDevice) ----------------------------------------------
    for case, bad in BAD_PER.items():
        add("mpcgpu_per_reset_dev", "per", "params " + case, 0, _ref(bad), P, P, None)
        add("mpcgpu_per_add_dev", "per", "params " + case, 0, _ref(bad), P, P, 0, 1, 0, None)
        add("mpcgpu_per_update_dev", "per", "params " + case, 0, _ref(bad), P, P, P, 1, None)
        add("mpcgpu_per_sample_dev", "per", "params " + case, 0, _ref(bad), P, P, 1, 1, P, P, P, None)
        add("mpcgpu_per_stats_dev", "per", "params " + case, 0, _ref(bad), P, P, P, None)

    # ---- plangpu.hip -----------------------------------------------------------------------------------------------------------
    def paths(params=plan_params(), B=4, **null):
        a = named(["rings", "start_goal", "status", "n_nodes", "nodes", "length"], **null)
        return (0, _ref(params), B, a["rings"], a["start_goal"], a["status"], a["n_nodes"], a["nodes"], a["length"], None)

    for case, bad in BAD_PLAN.items():
        add("mpcgpu_plan_record_doubles", "plan", "params " + case, _ref(bad))
        add("mpcgpu_plan_paths_dev", "plan", "params " + case, *paths(params=bad))
    for b in (0, -1):
        add("mpcgpu_plan_paths_dev", "plan", f"B {b}", *paths(B=b))
    for k in ("rings", "start_goal", "status", "n_nodes", "nodes", "length"):
        add("mpcgpu_plan_paths_dev", "plan", "null " + k, *paths(**{k: True}))
    add("mpcgpu_plan_paths_dev", "plan", "B 0, null rings", *paths(B=0, rings=True))

    # ---- mapgpu.hip ------------------------------------------------------------------------------------------------------------
    def draw(B=4, **null):
        a = named(["spec_table", "spare_ready", "attempt"], **null)
        return (0, B, 7, a["spec_table"], a["spare_ready"], a["attempt"], None)

    def rings(B=4, **null):
        a = named(["spec_table", "spare_ready", "rings", "start_goal"], **null)
        return (0, B, a["spec_table"], a["spare_ready"], a["rings"], a["start_goal"], None)
    record_ptrs = ["spec_table", "plan_status", "plan_n_nodes", "plan_nodes", "records2", "which", "spare_ready", "status"]

    def record(params=env_params(), B=4, **null):
        a = named(record_ptrs, **null)
        return (0, _ref(params), B, *(a[k] for k in record_ptrs), None)

    add("mpcgpu_map_draw_dev", "map", "B -1", *draw(B=-1))
    for k in ("spec_table", "spare_ready", "attempt"):
        add("mpcgpu_map_draw_dev", "map", "null " + k, *draw(**{k: True}))
    add("mpcgpu_map_rings_dev", "map", "B -1", *rings(B=-1))
    for k in ("spec_table", "spare_ready", "rings", "start_goal"):
        add("mpcgpu_map_rings_dev", "map", "null " + k, *rings(**{k: True}))
    for case, bad in BAD_ENV.items():
        add("mpcgpu_map_record_dev", "map", "params " + case, *record(params=bad))
    add("mpcgpu_map_record_dev", "map", "B -1", *record(B=-1))
    for k in record_ptrs:
        add("mpcgpu_map_record_dev", "map", "null " + k, *record(**{k: True}))

    # ---- dqngpu.hip ------------------------------------------------------------------------------------------------------------
    def minibatch(params=dqn_params(), n=32, **null):
        a = named(["state", "obs", "next_obs", "actions", "rewards", "dones", "grad", "loss"], **null)
        return (0, _ref(params), a["state"], a["obs"], a["next_obs"], a["actions"], a["rewards"], a["dones"], None, n, a["grad"],
                a["loss"], None, None)

    for entry in ("mpcgpu_dqn_grad_dev", "mpcgpu_dqn_step_dev"):
        for case, bad in BAD_DQN.items():
            add(entry, "dqn", "params " + case, *minibatch(params=bad))
        for n in (0, 257, -1):
            add(entry, "dqn", f"n {n}", *minibatch(n=n))
        for k in ("state", "obs", "next_obs", "actions", "rewards", "dones", "grad", "loss"):
            add(entry, "dqn", "null " + k, *minibatch(**{k: True}))
    for case, bad in BAD_DQN.items():
        add("mpcgpu_dqn_apply_dev", "dqn", "params " + case, 0, _ref(bad), P, P, 1.0, None)
    add("mpcgpu_dqn_apply_dev", "dqn", "null state", 0, _ref(dqn_params()), None, P, 1.0, None)
    add("mpcgpu_dqn_apply_dev", "dqn", "null grad", 0, _ref(dqn_params()), P, None, 1.0, None)
    ring = ["state", "buf_obs", "buf_next_obs", "buf_actions", "buf_rewards", "buf_dones", "losses"]

    def train(params=dqn_params(), size=1000, n=32, K=4, **null):
        a = named(ring, **null)
        return (0, _ref(params), *(a[k] for k in ring[:-1]), size, n, K, 1, 0, a["losses"], None)

    def train_per(dqn=dqn_params(), per=per_params(), n_entries=64, n=32, K=4, **null):
        a = named(ring + ["tree"], **null)
        return (0, _ref(dqn), _ref(per), a["state"], a["tree"], *(a[k] for k in ring[1:-1]), n_entries, n, K, 1, 0, a["losses"],
                None, None, None)

    for case, bad in BAD_DQN.items():
        add("mpcgpu_dqn_train_dev", "dqn", "params " + case, *train(params=bad))
        add("mpcgpu_dqn_train_per_dev", "dqn_per", "dqn " + case, *train_per(dqn=bad))
    for case, bad in BAD_PER.items():
        add("mpcgpu_dqn_train_per_dev", "dqn_per", "per " + case, *train_per(per=bad))
    add("mpcgpu_dqn_train_per_dev", "dqn_per", "dqn null, per null", *train_per(dqn=None, per=None))
    for n in (0, 257, -1):
        add("mpcgpu_dqn_train_dev", "dqn", f"n {n}", *train(n=n))
        add("mpcgpu_dqn_train_per_dev", "dqn_per", f"n {n}", *train_per(n=n))
    for K in (0, 65537, -1):
        add("mpcgpu_dqn_train_dev", "dqn", f"K {K}", *train(K=K))
        add("mpcgpu_dqn_train_per_dev", "dqn_per", f"K {K}", *train_per(K=K))
    for size in (0, -1, 2 ** 31):
        add("mpcgpu_dqn_train_dev", "dqn", f"size {size}", *train(size=size))
    for n_entries in (0, 65, -1):
        add("mpcgpu_dqn_train_per_dev", "dqn_per", f"n_entries {n_entries}", *train_per(n_entries=n_entries))
    for k in ring:
        add("mpcgpu_dqn_train_dev", "dqn", "null " + k, *train(**{k: True}))
    for k in ring + ["tree"]:
        add("mpcgpu_dqn_train_per_dev", "dqn_per", "null " + k, *train_per(**{k: True}))
    add("mpcgpu_dqn_train_per_dev", "dqn_per", "n 0, K 0, n_entries 0, null state", *train_per(n=0, K=0, n_entries=0, state=True))
    return out


def run(lib):
    """Every case once: [[entry, case, return code, text of the slot]]."""
    rows = []
    for entry, case, slot, call in cases(lib):
        rc = call()
        rows.append([entry, case, int(rc), getattr(lib, SLOTS[slot])().decode()])
    return rows


def dumps(rows) -> str:
    return json.dumps(rows, indent=0, ensure_ascii=True) + "\n"


def load(path=FIXTURE):
    with open(path) as fh:
        return json.load(fh)
