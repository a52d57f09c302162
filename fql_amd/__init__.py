"""fql_amd: MI355X-native (gfx950) Flow Q-Learning gradient step behind the reference's FQLAgent API.

`agents` mirrors the reference registry (agents/__init__.py:10-19) for the agents on the built path: FQL, IFQL, ReBRAC, SAC (RLPD's learner), BC
(flow-matching behavioural cloning), IQL, IQL-diffusion (the binary optimality family, sampled with classifier-free guidance) and CFGRL
(a goal-conditioned flow policy with a learned unconditional goal row, goals drawn from the row's own trajectory on the device): the
reference's eight keys.
"""
from .agent import FQLAgent, FQLAgentGroup, INFO_KEYS, NOISE_KEYS
from .config import get_config
from .datasets import Dataset, ReplayBuffer
from .ifql import IFQLAgent, IFQLAgentGroup, IFQL_INFO_KEYS
from .rebrac import ReBRACAgent, ReBRACAgentGroup, REBRAC_INFO_KEYS, REBRAC_CRITIC_INFO_KEYS
from .sac import SACAgent, SACAgentGroup, SAC_INFO_KEYS
from .bc import BCAgent, BC_INFO_KEYS, train_bc
from .iql import IQLAgent, IQLAgentGroup, IQL_INFO_KEYS
from .iql_diffusion import IQLDiffusionAgent, IQLDiffusionAgentGroup, IQLD_INFO_KEYS
from .cfgrl import CFGRLAgent, CFGRLAgentGroup, CFGRL_INFO_KEYS

agents = dict(fql=FQLAgent, ifql=IFQLAgent, rebrac=ReBRACAgent, sac=SACAgent, bc=BCAgent, iql=IQLAgent,
              iql_diffusion=IQLDiffusionAgent, cfgrl=CFGRLAgent)

__all__ = ['FQLAgent', 'FQLAgentGroup', 'IFQLAgent', 'IFQLAgentGroup', 'ReBRACAgent', 'ReBRACAgentGroup', 'SACAgent', 'SACAgentGroup', 'BCAgent', 'IQLAgent', 'IQLAgentGroup', 'IQLDiffusionAgent', 'IQLDiffusionAgentGroup', 'CFGRLAgent', 'CFGRLAgentGroup', 'train_bc', 'get_config', 'agents', 'INFO_KEYS', 'IFQL_INFO_KEYS',
           'REBRAC_INFO_KEYS', 'REBRAC_CRITIC_INFO_KEYS', 'SAC_INFO_KEYS', 'BC_INFO_KEYS', 'IQL_INFO_KEYS', 'IQLD_INFO_KEYS', 'CFGRL_INFO_KEYS', 'NOISE_KEYS', 'Dataset', 'ReplayBuffer']
