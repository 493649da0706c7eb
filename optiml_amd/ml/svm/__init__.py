__all__ = ['SVM', 'SVC', 'SVR', 'OneVsRestSVC', 'OneVsOneSVC', 'SVCGridSearchCV', 'MultiOutputSVR', 'SVRGridSearchCV',
           'CalibratedSVC', 'PairwiseCoupledSVC', 'OneClassSVM', 'one_class_nu_path', 'NuSVC', 'NuSVR',
           'nu_svc_path', 'nu_svr_path', 'OneVsOneNuSVC', 'ovo_nu_svc_path', 'NuSVCGridSearchCV', 'NuSVRGridSearchCV',
           'OneVsOneGridSearchCV', 'ovo_vote', 'RowSMOClassifier', 'RowSMORegression', 'RowOneClassSVM', 'RowNuSVC', 'RowNuSVR']

from ._base import SVM, SVC, SVR
from .smo_rows import RowSMOClassifier, RowSMORegression
from .multiclass import OneVsRestSVC
from .onevsone import OneVsOneSVC
from .model_selection import SVCGridSearchCV, SVRGridSearchCV
from .multioutput import MultiOutputSVR
from .calibration import CalibratedSVC
from .coupling import PairwiseCoupledSVC
from .oneclass import OneClassSVM, one_class_nu_path
from .nu import NuSVC, NuSVR, nu_svc_path, nu_svr_path
from .nu_rows import RowOneClassSVM, RowNuSVC, RowNuSVR
from .nu_ovo import OneVsOneNuSVC, ovo_nu_svc_path
from .nu_search import NuSVCGridSearchCV, NuSVRGridSearchCV
from .ovo_search import OneVsOneGridSearchCV, ovo_vote
