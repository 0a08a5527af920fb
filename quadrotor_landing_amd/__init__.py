"""MI355X-native batched relative-pose EKF engine (drop-in for the hot path of
mbrymer/quadrotor_landing's quad_state_estimation filter core)."""
from ._lib import LIB_PATH, QLE_F32, QLE_F64, QleDerived, QleError, QleParams, QleSynthCfg, launch_census, lib, side_launch_census  # noqa: F401
from .ekf import BatchedRelativePoseEKF, InputSequence  # noqa: F401
from .twin import RelativePoseEKF  # noqa: F401
from .devio import DeviceIO  # noqa: F401
from .params import default_params, derive, load_yaml, make_params, set_fields  # noqa: F401
from . import replay  # noqa: F401
from . import adapt  # noqa: F401
from . import bank  # noqa: F401
from . import budget  # noqa: F401
from . import consistency  # noqa: F401
from . import health  # noqa: F401
from . import imm  # noqa: F401
from . import lookahead  # noqa: F401
from . import score  # noqa: F401
from . import sequence  # noqa: F401
from . import stateio  # noqa: F401
from .sequence import DeviceSequence, SequenceResult  # noqa: F401
from .budget import Budget  # noqa: F401
