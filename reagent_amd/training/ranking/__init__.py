from .helper import ips_clamp  # noqa: F401
from .seq2slate_trainer import Seq2SlateTrainer  # noqa: F401
