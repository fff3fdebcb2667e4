"""Aid embeddings behind the reference's ``src/gensim_fasttext`` module surface: skip-gram negative-sampling training on
the device (``skipgram``) and the ``trainer`` command line that reads the reference's fastText and Word2Vec YAML files."""
from .skipgram import (BATCH, HOGWILD, SkipGramEngine, init_tables, learning_rate, load_vec, save_vec, train,  # noqa: F401
                       vocab_tables)
