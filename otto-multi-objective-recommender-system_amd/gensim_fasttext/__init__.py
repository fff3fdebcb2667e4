"""Aid embeddings behind the reference's ``src/gensim_fasttext`` module surface: skip-gram, CBOW and Doc2Vec training on
the device (``skipgram``) and the ``trainer`` command line that reads the reference's fastText, Word2Vec and Doc2Vec YAML
files."""
from .skipgram import (ARCH_CBOW, ARCH_DBOW, ARCH_PVDM, BATCH, CBOW_FASTTEXT, CBOW_MEAN, CBOW_SUM, HOGWILD,  # noqa: F401
                       SkipGramEngine, init_doc, init_tables, learning_rate, load_vec, save_vec, train, train_cbow,
                       train_doc2vec, vocab_tables)
