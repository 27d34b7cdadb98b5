"""The acting side of the policy-gradient trainers: Policy(scorer, sampler) and the softmax sampler they are built from
(reagent/gym/policies/).  Torch code: acting is outside the training step, whose log-softmax, log-probability and entropy
run in rg_pg_head; the trainers read `sampler.temperature` every step."""
from .policy import Policy  # noqa: F401
from .samplers.discrete_sampler import SoftmaxActionSampler  # noqa: F401
from .cem_policy import CEMPolicy  # noqa: F401
