"""Mirror of the reference's params package, as far as the header rules read it.

    ChainConfig                      params/config.go:103-124 (the fields the ethash header rules read)
    MainnetChainConfig .. TestChainConfig    params/config.go:33-94
    CliqueConfig                     params/config.go:134-138
    DAOForkBlockExtra, DAOForkExtraRange     params/dao.go:28, :32
    the protocol constants           params/protocol_params.go

A fork block of None is the reference's nil big.Int: the fork never happens.
"""
from __future__ import annotations

from . import _lib

MaximumExtraDataSize = 32
GasLimitBoundDivisor = 1024
MinGasLimit = 5000
DifficultyBoundDivisor = 2048
MinimumDifficulty = 131072
DurationLimit = 13

DAOForkBlockExtra = bytes.fromhex("64616f2d686172642d666f726b")  # "dao-hard-fork"
DAOForkExtraRange = 10


class CliqueConfig:
    """params.CliqueConfig: Period, the seconds between blocks to enforce; Epoch, the epoch length to reset votes and
    checkpoint (0: the engine's default of 30000, clique.go:216-218)"""

    def __init__(self, Period=0, Epoch=0):
        self.Period, self.Epoch = int(Period), int(Epoch)
        if not (0 <= self.Period < 1 << 64 and 0 <= self.Epoch < 1 << 64):
            raise ValueError("params: Period and Epoch are uint64")

    def as_struct(self) -> "_lib.CliqueConfigStruct":
        """gsv_clique_config (include/gsv.h), as given: the engine defaults the epoch"""
        return _lib.CliqueConfigStruct(self.Period, self.Epoch)


class ChainConfig:
    def __init__(self, ChainId=None, HomesteadBlock=None, DAOForkBlock=None, DAOForkSupport=False, EIP150Block=None,
                 EIP150Hash=bytes(32), EIP155Block=None, EIP158Block=None, ByzantiumBlock=None,
                 ConstantinopleBlock=None, Clique=None):
        self.Clique = Clique
        self.ChainId = ChainId
        self.HomesteadBlock = HomesteadBlock
        self.DAOForkBlock = DAOForkBlock
        self.DAOForkSupport = bool(DAOForkSupport)
        self.EIP150Block = EIP150Block
        self.EIP150Hash = bytes(EIP150Hash)
        self.EIP155Block = EIP155Block
        self.EIP158Block = EIP158Block
        self.ByzantiumBlock = ByzantiumBlock
        self.ConstantinopleBlock = ConstantinopleBlock
        if len(self.EIP150Hash) != 32:
            raise ValueError("params: EIP150Hash is 32 bytes")
        for name in ("HomesteadBlock", "DAOForkBlock", "EIP150Block", "ByzantiumBlock"):
            v = getattr(self, name)
            if v is not None and not 0 <= int(v) < 1 << 64:
                raise ValueError("params: %s is a block number below 2^64" % name)

    @staticmethod
    def _forked(s, head) -> bool:  # isForked, params/config.go:234-239
        return s is not None and head is not None and int(s) <= int(head)

    def IsHomestead(self, num) -> bool:
        return self._forked(self.HomesteadBlock, num)

    def IsByzantium(self, num) -> bool:
        return self._forked(self.ByzantiumBlock, num)

    def as_struct(self) -> "_lib.ChainConfigStruct":
        """gsv_chain_config (include/gsv.h)"""
        st = _lib.ChainConfigStruct()
        for field, flag, v in (("homestead_block", "has_homestead", self.HomesteadBlock),
                               ("dao_fork_block", "has_dao_fork", self.DAOForkBlock),
                               ("eip150_block", "has_eip150", self.EIP150Block),
                               ("byzantium_block", "has_byzantium", self.ByzantiumBlock)):
            setattr(st, field, 0 if v is None else int(v))
            setattr(st, flag, 0 if v is None else 1)
        st.dao_fork_support = int(self.DAOForkSupport)
        for k in range(32):
            st.eip150_hash[k] = self.EIP150Hash[k]
        return st


MainnetChainConfig = ChainConfig(
    ChainId=1, HomesteadBlock=1150000, DAOForkBlock=1920000, DAOForkSupport=True, EIP150Block=2463000,
    EIP150Hash=bytes.fromhex("2086799aeebeae135c246c65021c82b4e15a2c451340993aacfd2751886514f0"), EIP155Block=2675000,
    EIP158Block=2675000, ByzantiumBlock=4370000)

TestnetChainConfig = ChainConfig(
    ChainId=3, HomesteadBlock=0, DAOForkBlock=None, DAOForkSupport=True, EIP150Block=0,
    EIP150Hash=bytes.fromhex("41941023680923e0fe4d74a34bdac8141f2540e3ae90623718e47d66d1ca4a2d"), EIP155Block=10,
    EIP158Block=10, ByzantiumBlock=1700000)

RinkebyChainConfig = ChainConfig(
    ChainId=4, HomesteadBlock=1, DAOForkBlock=None, DAOForkSupport=True, EIP150Block=2,
    EIP150Hash=bytes.fromhex("9b095b36c15eaf13044373aef8ee0bd3a382a5abb92e402afa44b8249c3a90e9"), EIP155Block=3,
    EIP158Block=3, ByzantiumBlock=1035301, Clique=CliqueConfig(Period=15, Epoch=30000))

AllEthashProtocolChanges = ChainConfig(ChainId=1337, HomesteadBlock=0, DAOForkBlock=None, DAOForkSupport=False,
                                       EIP150Block=0, EIP155Block=0, EIP158Block=0, ByzantiumBlock=0)

AllCliqueProtocolChanges = ChainConfig(ChainId=1337, HomesteadBlock=0, DAOForkBlock=None, DAOForkSupport=False,
                                       EIP150Block=0, EIP155Block=0, EIP158Block=0, ByzantiumBlock=0,
                                       Clique=CliqueConfig(Period=0, Epoch=30000))

TestChainConfig = ChainConfig(ChainId=1, HomesteadBlock=0, DAOForkBlock=None, DAOForkSupport=False, EIP150Block=0,
                              EIP155Block=0, EIP158Block=0, ByzantiumBlock=0)

__all__ = ["ChainConfig", "CliqueConfig", "MainnetChainConfig", "TestnetChainConfig", "RinkebyChainConfig",
           "AllEthashProtocolChanges", "AllCliqueProtocolChanges", "TestChainConfig", "DAOForkBlockExtra",
           "DAOForkExtraRange", "MaximumExtraDataSize", "GasLimitBoundDivisor",
           "MinGasLimit", "DifficultyBoundDivisor", "MinimumDifficulty", "DurationLimit"]
