__all__ = ['SVM', 'SVC', 'SVR', 'OneVsRestSVC']

from ._base import SVM, SVC, SVR
from .multiclass import OneVsRestSVC
