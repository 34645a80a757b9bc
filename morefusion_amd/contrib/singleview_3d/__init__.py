# flake8: noqa
from . import models
from .evaluate import METHODS, evaluate_batch
