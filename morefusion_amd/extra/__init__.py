# flake8: noqa
from . import _torch as torch_
from ._torch import median
from . import _open3d as open3d
from ._render import render_cad
