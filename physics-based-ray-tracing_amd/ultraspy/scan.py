"""USMain.py:9"""
from ..beamform import GridScan, PolarScan  # noqa: F401
