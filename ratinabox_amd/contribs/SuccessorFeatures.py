"""`SuccessorFeatures` — the successor features of a set of features, learned on the device (reference
ratinabox/contribs/SuccessorFeatures.py): a `ValueNeuron` with one value neuron per feature whose reward IS the
features' firing rate.  `params["features"]` is any population of the same Agent; `params["input_layers"]` are the basis
features the successor features are a weighted sum of.  `update_weights()` hands the features' device-resident last
rates `[n][B_padded]` to the TD kernel as they are: one reward per (neuron, agent), no copy.  Like the reference,
`update()` does not update the features or the basis features: the loop does.  In a `StepPlan` the reward is this step's
row of the features, which must be recorded in the plan before the learner."""
import copy

from .. import _lib as _L
from .ValueNeuron import ValueNeuron


class SuccessorFeatures(ValueNeuron):
    default_params = {
        "features": None,   # the population whose successor features are learned
        "name": "SuccessorFeatures",
    }

    def __init__(self, Agent, params={}):
        self.params = copy.deepcopy(__class__.default_params)
        self.params.update(params)
        if self.params["features"] is None:
            raise Exception("The input parameter dictionary must contain features to calculate the successor features "
                            "for: params['features'] = any Neurons population (PlaceCells, BoundaryVectorCells, ...).")
        self.params["n"] = self.params["features"].n
        super().__init__(Agent, self.params)

    def update_weights(self):
        super().update_weights(self.params["features"]._rates)

    def learn(self, **kwargs):
        """`update(); update_weights()` with the trace update riding in the gradient kernel (ValueNeuron.learn)."""
        super().learn(self.params["features"]._rates, **kwargs)

    def _plan_reward(self, plan_index):
        feats = self.params["features"]
        if feats not in plan_index:
            raise NotImplementedError(f"the features {feats.name} must be recorded in the plan before {self.name}")
        return _L.REWARD_POPULATION, plan_index[feats]
