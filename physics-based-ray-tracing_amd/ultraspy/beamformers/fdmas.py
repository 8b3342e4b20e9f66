"""ultraspy.beamformers.fdmas (DESIGN D19)"""
from ...beamform import FilteredDelayMultiplyAndSum  # noqa: F401
