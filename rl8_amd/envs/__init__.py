"""The reference's example environments (``examples/*/env.py``) as batched HIP kernels."""

from .algotrading import AlgoTrading
from .algotrading_models import LSTMTrader
from .cartpole import CartPole, CartPoleConfig
from .mountain_car import MountainCar, MountainCarConfig
from .pendulum import Pendulum, PendulumConfig

__all__ = ["AlgoTrading", "CartPole", "CartPoleConfig", "LSTMTrader", "MountainCar", "MountainCarConfig", "Pendulum",
           "PendulumConfig"]
