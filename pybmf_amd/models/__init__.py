from .BaseModel import BaseModel
from .ContinuousModel import ContinuousModel
from .BinaryMFPenalty import BinaryMFPenalty
from .WNMF import WNMF
from .PNLPF import PNLPF
from .BinaryMFThreshold import BinaryMFThreshold
from .ELBMF import ELBMF
from .PRIMP import PRIMP
from .FastStep import FastStep
from .BooleanModel import BooleanModel
from .GreConD import GreConD
from .GreConDPlus import GreConDPlus
from .Asso import Asso
from .AssoIter import AssoIter
from .AssoOpt import AssoOpt
from .MEBF import MEBF
from .Panda import Panda
from .Hyper import Hyper
from .HyperPlus import HyperPlus
from .NMFSklearn import NMFSklearn
from .SimpleThreshold import SimpleThreshold
from .BinaryMFThresholdExColumnwise import BinaryMFThresholdExColumnwise
from .MessagePassing import MessagePassing

__all__ = ["BaseModel", "ContinuousModel", "BinaryMFPenalty", "PNLPF", "WNMF", "BinaryMFThreshold", "ELBMF", "PRIMP", "FastStep", "BooleanModel", "GreConD", "GreConDPlus", "Asso", "AssoIter", "AssoOpt", "MEBF", "Panda", "Hyper", "HyperPlus", "NMFSklearn", "SimpleThreshold", "BinaryMFThresholdExColumnwise", "MessagePassing"]
