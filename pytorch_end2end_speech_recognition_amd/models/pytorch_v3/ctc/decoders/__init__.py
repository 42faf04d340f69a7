from .beam_search_decoder import BeamSearchDecoder  # noqa: F401
from .greedy_decoder import GreedyDecoder  # noqa: F401
