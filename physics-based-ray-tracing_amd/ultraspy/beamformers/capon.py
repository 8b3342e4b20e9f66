"""ultraspy.beamformers.capon (DESIGN D23)"""
from ...beamform import Capon  # noqa: F401
