"""stochastic-inventory_amd -- MI355X-native engine for the finite-horizon SDP recursion of
RobinChen121/Stochastic-Inventory's src/sdp (hand-written HIP behind the C ABI of include/sdpgpu.h).

The directory name carries a hyphen (it is fixed by the build contract); import it as
`stochastic_inventory_amd` through the alias module at the repository root.
"""
from . import _abi
from ._abi import (FAMILY_BACKORDER, FAMILY_CASH, FAMILY_CASH_LEADTIME, FAMILY_LEADTIME, FAMILY_OVERDRAFT,
                   FAMILY_STAFF, FAMILY_SURVIVAL, KERNEL_AUTO, KERNEL_GATHER, KERNEL_WINDOW, SdpgpuBatchPlan, SdpgpuBatchStaffPlan, SdpgpuBatchStats, SdpgpuConvexity, SdpgpuDesc, SdpgpuError, SdpgpuStats, desc_defaults)
from .batch import SdpBatch, StaffBatch
from .engine import SdpEngine
from .fitss import FindsSOverDraft, FitsS
from .functors import (BackorderFunctor, CashFunctor, CashXRFunctor, CashLeadtimeFunctor, CustomFunctor, LeadtimeFunctor, OverdraftFunctor,
                       SurvivalFunctor, java_round)
from .multiitem import (Actions, CashRecursionMulti, CashRecursionMultiLead, CashRecursionMultiXR, CashSimulationMulti,
                        CashSimulationMultiXR, CashStateMulti, CashStateMultiLead, CashStateMultiXR, MultiLeadResult, MultiPolicy,
                        multicash_solve, multilead_solve, multixr_solve,
                        CashRecursionV, CashStateMultiYR, CashStateR, MultiVResult, multiv_alpha_list, multiv_solve)
from .pmf import BinomialDist, DiscreteDistribution, GammaDist, GetPmf, NormalDist, PoissonDist, UniformIntDist, staff_level_pmf
from .recursion import (CLSP, CashLeadtimeRecursion, CashRecursion, CashRecursionXR, LeadtimeRecursion, Recursion, RecursionBatch, RecursionG,
                        RiskRecursion)
from .simulation import CashSimulation, CashSimulationXR, RiskSimulation, Sampling, SimulateFitsS, Simulation, SimulationBatch
from .workforce import SimulatesS, StaffFunctor, StaffRecursion, StaffRecursionBatch, StaffState
from .structure import CheckKConvexity
from . import cash_structure
from .cash_structure import CashStructure
from .states import CashLeadtimeState, CashState, CashStateXR, LeadtimeState, OptDirection, RiskState, State

__all__ = [
    "SdpEngine", "SdpBatch", "SdpgpuBatchPlan", "SdpgpuBatchStats", "RecursionBatch", "SdpgpuDesc", "SdpgpuError", "SdpgpuStats", "desc_defaults",
    "BackorderFunctor", "LeadtimeFunctor", "CashFunctor", "CashXRFunctor", "OverdraftFunctor", "CashLeadtimeFunctor", "SurvivalFunctor", "CustomFunctor",
    "Recursion", "CLSP", "LeadtimeRecursion", "CashRecursion", "CashRecursionXR", "CashLeadtimeRecursion", "RiskRecursion",
    "StaffRecursion", "StaffRecursionBatch", "StaffBatch", "SdpgpuBatchStaffPlan", "StaffFunctor", "StaffState", "SimulatesS", "BinomialDist", "staff_level_pmf",
    "multilead_solve", "multicash_solve", "multixr_solve", "MultiLeadResult", "Actions", "CashRecursionMulti",
    "CashRecursionMultiLead", "CashRecursionMultiXR", "CashStateMulti", "CashStateMultiLead", "CashStateMultiXR",
    "MultiPolicy", "CashSimulationMulti", "CashSimulationMultiXR",
    "multiv_solve", "multiv_alpha_list", "MultiVResult", "CashRecursionV", "CashStateMultiYR", "CashStateR",
    "GetPmf", "PoissonDist", "GammaDist", "NormalDist", "UniformIntDist", "DiscreteDistribution", "Simulation", "SimulationBatch", "RiskSimulation", "CashSimulation", "CashSimulationXR", "RecursionG", "Sampling",
    "FitsS", "FindsSOverDraft", "SimulateFitsS", "CheckKConvexity", "SdpgpuConvexity", "CashStructure", "cash_structure",
    "State", "LeadtimeState", "CashState", "CashStateXR", "CashLeadtimeState", "RiskState", "OptDirection", "java_round",
]
