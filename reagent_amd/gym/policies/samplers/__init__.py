from .discrete_sampler import SoftmaxActionSampler  # noqa: F401
