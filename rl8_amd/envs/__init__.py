"""The reference's example environments (``examples/*/env.py``) as batched HIP kernels."""

from .algotrading import AlgoTrading
from .algotrading_models import LSTMTrader, MLPTrader, TransformerTrader
from .cartpole import CartPole, CartPoleConfig
from .mountain_car import MountainCar, MountainCarConfig
from .pendulum import Pendulum, PendulumConfig

__all__ = ["AlgoTrading", "CartPole", "CartPoleConfig", "LSTMTrader", "MLPTrader", "MountainCar", "MountainCarConfig",
           "Pendulum", "PendulumConfig", "TransformerTrader"]
