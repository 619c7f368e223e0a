from .acting import ActResult
from .baselines import DDPG_LA, SAC_LA
from .evaluation import BestPolicy, ConstraintReport, EvalCurve, EvalResult, EvalTrajectory, OpfGap, curve_seed, evaluate_filtered, evaluate_opf, opf_gap
from .pretrain import Demonstrations, PretrainResult
from .rpo_ddpg import RPODDPG
from .rpo_sac import RPOSAC
from .trainer import NonFiniteError

__all__ = ["RPODDPG", "DDPG_LA", "RPOSAC", "SAC_LA", "NonFiniteError", "EvalResult", "EvalTrajectory", "ConstraintReport", "EvalCurve", "BestPolicy", "curve_seed", "ActResult", "OpfGap", "opf_gap", "evaluate_opf", "evaluate_filtered", "Demonstrations", "PretrainResult"]
