"""
fcdiff_amd -- the fcdiff fit path on MI355X (gfx950).

Same public names as the reference package (fcdiff/__init__.py:1-5):
    UnsharedRegionModel, fit (module), N_to_C, nm_to_c, c_to_nm
and the shared-region model the reference names but does not ship: SharedRegionModel, fit.SharedRegionFit;
between the two, one anomaly map per known group of patients: GroupedRegionModel, fit.GroupedRegionFit; and with the groups
unknown -- latent subtypes of patients, found by the fit: SubtypeRegionModel, fit.SubtypeRegionFit.
covariates (module): adjustment of the connections for subject covariates fitted on the controls, in front of a fit.
baseline (module): the classical analyses beside the models -- normative z-scores per patient, permutation group tests.
The fitter runs hand-written HIP kernels through the C ABI of include/fcdiff_hip.h; there is no CPU
fallback: using the fitter without libfcdiff_hip.so or without a GPU raises.
"""
from .model import UnsharedRegionModel, SharedRegionModel, GroupedRegionModel, SubtypeRegionModel
from . import fit
from . import covariates
from . import baseline
from . import util
from .util import N_to_C, nm_to_c, c_to_nm

__all__ = ["UnsharedRegionModel", "SharedRegionModel", "GroupedRegionModel", "SubtypeRegionModel", "fit", "covariates", "baseline", "util", "N_to_C", "nm_to_c", "c_to_nm"]
