"""ultraspy.beamformers.pdas (DESIGN D19)"""
from ...beamform import PDelayAndSum  # noqa: F401
