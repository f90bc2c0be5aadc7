"""cfm_amd — MI355X (gfx950) native minibatch-OT coupling + CFM sampling, behind the
TorchCFM API (``torchcfm.OTPlanSampler`` / ``ConditionalFlowMatcher`` family).

    import cfm_amd as torchcfm
    from cfm_amd.conditional_flow_matching import ExactOptimalTransportConditionalFlowMatcher
    from cfm_amd.optimal_transport import OTPlanSampler, wasserstein
    from cfm_amd.models import MLP
"""
from .conditional_flow_matching import *  # noqa: F401,F403
from .conditional_flow_matching import (  # noqa: F401
    ConditionalFlowMatcher,
    DSBMConditionalFlowMatcher,
    ExactOptimalTransportConditionalFlowMatcher,
    ScheduledBridgeConditionalFlowMatcher,
    SchrodingerBridgeConditionalFlowMatcher,
    TargetConditionalFlowMatcher,
    VariancePreservingConditionalFlowMatcher,
    pad_t_like_x,
)
from .models import MLP  # noqa: F401
from .schedule import (  # noqa: F401
    ConstantNoiseScheduler,
    CosineNoiseScheduler,
    LinearDecreasingNoiseScheduler,
    NoiseScheduler,
)
from .cnf import CNF, AugmentationModule, DifferentiableCNF, RegularizedCNF, log_likelihood  # noqa: F401
from .ode import AdaptiveDifferentiableNeuralODE, DifferentiableNeuralODE  # noqa: F401
from .action_matching import action_matching_loss  # noqa: F401
from .icnn import ICNN, icnn_f_loss, icnn_g_loss, icnn_w2  # noqa: F401
from .optim import FusedAdam  # noqa: F401
from .train import DSBMStep, RegressionStep, SF2MStep  # noqa: F401
from .sde import DSBMFlowSolver, FlowSolver  # noqa: F401
from .optimal_transport import OTPlanSampler, wasserstein  # noqa: F401
from .trajectory import TrajectoryFlowMatcher  # noqa: F401

__version__ = "0.1.0"
