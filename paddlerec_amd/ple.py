"""Host-side mirror of the reference's PLE plugin (models/multitask/ple/net.py:20-224 PLELayer / SinglePLELayer,
dygraph_model.py) on the recengine HIP kernels: Progressive Layered Extraction — level_number CGC levels of task experts,
shared experts, one gate per task and (below the last level) a shared gate — over the census features, two tasks.

A level is expert slots and gates over task_num + 1 inputs (mtl.py): task gate i mixes its own exp_per_task slots, then the
shared_num shared slots (two slot ranges of rec_mtl_mix_fwd); the shared gate mixes every slot.  Level 0 reads the features
on every input: one packed image, one GEMM.  A level >= 1 has one image per input.  Kept as the reference writes it,
the expert indexing included (QUIRKS; slot_map() prints the map)."""
from .mtl import MtlDygraphModel, MtlLayer

QUIRKS = ("task i's expert j is _param_expert[i * task_num + j], not i * exp_per_task + j (net.py:182): with the shipped 2 "
          "tasks x 3 experts, task 0 runs exp_0_0, exp_0_1, exp_0_2 and task 1 runs exp_0_2 (again, on its own input), "
          "exp_1_0, exp_1_1; exp_1_2 is never called, has no gradient and never moves; exp_0_2 fills two slots and its "
          "gradient is the sum of both; a config whose index runs past the expert list is refused (the reference raises "
          "IndexError in forward); expert constants are 10^-(1 + i * exp_per_task + j), shared experts and gates 10^-(i+1), "
          "the shared gate 0.1, every bias 0.1; the shared gate is registered under two names (lev_L_gate_shared_ and "
          "_param_gate_shared), both in the state_dict; the softmax outputs are clipped to [1e-15, 1 - 1e-15] in float32, "
          "where the upper bound is 1; only column 1 of a prediction enters the loss (log_loss, epsilon 1e-4) and the AUC; "
          "the data's label columns are marital, income while the outputs are income, marital; Adam (beta 0.9 / 0.999, "
          "epsilon 1e-8, non-lazy) at hyper_parameters.optimizer.learning_rate")


def expert_names(lev, task_num, exp_per_task, shared_num):
    """_param_expert of level lev in construction order (net.py:115-146), as state_dict prefixes."""
    pre = "lev_%d.lev_%d_exp_" % (lev, lev)
    return [pre + "%d_%d" % (i, j) for i in range(task_num) for j in range(exp_per_task)] + \
           [pre + "shared_%d" % i for i in range(shared_num)]


def ple_plan(feature_size, task_num, exp_per_task, shared_num, expert_size, tower_size, level_number):
    """The mtl.py plan of PLELayer(feature_size, task_num, exp_per_task, shared_num, expert_size, tower_size, level_number)."""
    F, T, P, Sh, S, L = (int(v) for v in (feature_size, task_num, exp_per_task, shared_num, expert_size, level_number))
    if min(F, T, P, Sh, S, L, int(tower_size)) < 1:
        raise ValueError("PLE: feature_size, task_num, exp_per_task, shared_num, expert_size, tower_size and level_number must "
                         "be positive (shared_num 0 breaks the reference's expert_outputs[-shared_num:])")
    last = (T - 1) * T + P - 1                                  # the largest index net.py:182 forms
    if last >= T * P + Sh:
        raise ValueError("PLE: task_num %d, exp_per_task %d, shared_num %d: the reference indexes its task experts as "
                         "_param_expert[i * task_num + j] (net.py:182), which reaches %d past the %d experts of a level — "
                         "its forward raises IndexError" % (T, P, Sh, last, T * P + Sh))
    params, aliases, levels = [], {}, []
    for lev in range(L):
        K = F if lev == 0 else S
        names = expert_names(lev, T, P, Sh)
        for i in range(T):
            for j in range(P):
                params.append((names[i * P + j], K, S, 10.0 ** -(1 + i * P + j), 0.1))
        for i in range(Sh):
            params.append((names[T * P + i], K, S, 10.0 ** -(i + 1), 0.1))
        gate = "lev_%d.lev_%d_gate_" % (lev, lev)
        for i in range(T):
            params.append((gate + str(i), K, P + Sh, 10.0 ** -(i + 1), 0.1))
        slots = [(names[i * T + j], i) for i in range(T) for j in range(P)]        # net.py:180-185, as written
        slots += [(names[P * T + i], T) for i in range(Sh)]
        n = len(slots)
        gates = [(gate + str(i), i, (i * P, P, n - Sh, Sh)) for i in range(T)]
        if lev != L - 1:
            params.append((gate + "shared_", K, n, 0.1, 0.1))
            aliases["lev_%d._param_gate_shared" % lev] = gate + "shared_"
            gates.append((gate + "shared_", T, (0, n, 0, 0)))
        levels.append(dict(slots=slots, gates=gates))
    for i in range(T):
        c = 10.0 ** -(i + 1)
        params += [("tower_%d" % i, S, int(tower_size), c, 0.1), ("tower_out_%d" % i, int(tower_size), 2, c, 0.1)]
    return dict(params=params, aliases=aliases, levels=levels, n_inputs=T + 1, tasks=T)


class PLELayer(MtlLayer):
    """ple/net.py:20-101.  forward(input_data [B, feature_size]) -> task_num predictions [B, 2]."""

    def __init__(self, feature_size, task_num, exp_per_task, shared_num, expert_size, tower_size, level_number, device="cuda",
                 kernels=None):
        super().__init__(ple_plan(feature_size, task_num, exp_per_task, shared_num, expert_size, tower_size, level_number),
                         device, kernels)
        self.task_num, self.exp_per_task, self.shared_num = task_num, exp_per_task, shared_num
        self.expert_size, self.tower_size, self.level_number = expert_size, tower_size, level_number

    def slot_map(self, level=0):
        """[(slot, expert name, input)] of a level: which Linear fills which column block of H, on which input."""
        return [(e, n, i) for e, (n, i) in enumerate(self.plan["levels"][level]["slots"])]

    def unused(self):
        """The state_dict prefixes of the Linears forward() never calls."""
        return [n for n, _, _, _, _ in self.plan["params"] if n + ".weight" not in self._views["g"]]


class DygraphModel(MtlDygraphModel):
    """ple/dygraph_model.py — same method names."""

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return PLELayer(g("hyper_parameters.feature_size"), g("hyper_parameters.task_num"), g("hyper_parameters.exp_per_task"),
                        g("hyper_parameters.shared_num"), g("hyper_parameters.expert_size"), g("hyper_parameters.tower_size"),
                        g("hyper_parameters.level_number"), device=device, kernels=kernels)
