__all__ = ['SVM', 'SVC', 'SVR', 'OneVsRestSVC', 'SVCGridSearchCV']

from ._base import SVM, SVC, SVR
from .multiclass import OneVsRestSVC
from .model_selection import SVCGridSearchCV
