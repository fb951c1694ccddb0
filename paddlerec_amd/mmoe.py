"""Host-side mirror of the reference's MMoE plugin (models/multitask/mmoe/net.py:20-109 MMoELayer, dygraph_model.py) on the
recengine HIP kernels: Multi-gate Mixture-of-Experts over the census features, two tasks (income, marital).

expert_num experts Linear(feature_size, expert_size) + ReLU and gate_num gates Linear(feature_size, expert_num) + softmax
read the same features: ONE packed image [feature_size, expert_num * expert_size + gate_num * expert_num], one GEMM
(mtl.py).  Gate g's mixture (rec_mtl_mix_fwd; every gate mixes all experts, one slot range) feeds tower_g (ReLU) ->
tower_out_g -> softmax -> clip (rec_mtl_head).  Kept as the reference writes it (QUIRKS)."""
from .mtl import MtlDygraphModel, MtlLayer

QUIRKS = ("weights are constants, 10^-(i+1) for expert i and for gate i, every bias 0.1; tower_i and tower_out_i start from "
          "the GATE's constant 10^-(i+1) (net.py:62-83 reuse gate_init); the softmax outputs are clipped to [1e-15, 1 - 1e-15] "
          "in float32, where the upper bound is 1; only column 1 of a prediction enters the loss (log_loss, epsilon 1e-4) "
          "and the AUC; the data's label columns are marital, income while the outputs are income, marital; Adam (beta "
          "0.9 / 0.999, epsilon 1e-8, non-lazy) at hyper_parameters.optimizer.learning_rate")


def mmoe_plan(feature_size, expert_num, expert_size, tower_size, gate_num):
    """The mtl.py plan of MMoELayer(feature_size, expert_num, expert_size, tower_size, gate_num)."""
    F, E, S, G = int(feature_size), int(expert_num), int(expert_size), int(gate_num)
    if min(F, E, S, G, int(tower_size)) < 1:
        raise ValueError("MMoE: feature_size, expert_num, expert_size, tower_size and gate_num must be positive")
    params = [("expert_%d" % i, F, S, 10.0 ** -(i + 1), 0.1) for i in range(E)]
    for i in range(G):
        c = 10.0 ** -(i + 1)
        params += [("gate_%d" % i, F, E, c, 0.1), ("tower_%d" % i, S, int(tower_size), c, 0.1), ("tower_out_%d" % i, int(tower_size), 2, c, 0.1)]
    level = dict(slots=[("expert_%d" % i, 0) for i in range(E)], gates=[("gate_%d" % i, 0, (0, E, 0, 0)) for i in range(G)])
    return dict(params=params, aliases={}, levels=[level], n_inputs=1, tasks=G)


class MMoELayer(MtlLayer):
    """mmoe/net.py:20-109.  forward(input_data [B, feature_size]) -> gate_num predictions [B, 2]."""

    def __init__(self, feature_size, expert_num, expert_size, tower_size, gate_num, device="cuda", kernels=None):
        super().__init__(mmoe_plan(feature_size, expert_num, expert_size, tower_size, gate_num), device, kernels)
        self.expert_num, self.expert_size, self.tower_size, self.gate_num = expert_num, expert_size, tower_size, gate_num


class DygraphModel(MtlDygraphModel):
    """mmoe/dygraph_model.py — same method names."""

    def create_model(self, config, device="cuda", kernels=None):
        g = config.get
        return MMoELayer(g("hyper_parameters.feature_size", None), g("hyper_parameters.expert_num", None),
                         g("hyper_parameters.expert_size", None), g("hyper_parameters.tower_size", None),
                         g("hyper_parameters.gate_num", None), device=device, kernels=kernels)
