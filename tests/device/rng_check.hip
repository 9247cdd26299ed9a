// TEST-ONLY: every function of curdleproofs_amd/csrc/rng.hpp (the ChaCha12 block, the word stream, the samplers, the key expansion and the
// split) on raw words, one source compiled twice:
//   g++ -x c++ ...                     -> the host twin: every operation in a plain loop over the rows
//   hipcc --offload-arch=gfx950 ...    -> the device program: every operation in a kernel of its own, one thread per row, 64-thread blocks
// tests/test_rng_check_cpu.py and tests/test_gpu_rng.py feed both the same rows (tests/rng_cases.py) and compare the results with each other
// and with the Python model (tests/stdrng_ref.py).  Nothing in curdleproofs_amd/ links it.
//
// The command line, the record format, the exit codes and the runner are those of check_harness.hpp; --list prints name, input words per
// row, output words per row.  A state travels as ten words: key[8], word_pos low, high.
#define CHECK_PROG "rng_check"
#include "check_harness.hpp"
#include "../../curdleproofs_amd/csrc/rng.hpp"

using namespace cpx;

CPX_HD void st_pos(uint32_t* out, uint64_t pos) {
  out[0] = (uint32_t)pos;
  out[1] = (uint32_t)(pos >> 32);
}
constexpr int CHK_U32 = 40, CHK_U64 = 20, CHK_FR = 4, CHK_SHUFFLE = 40;

OP(Block, 10, 16, chacha12_block(in, (uint64_t)in[8] | ((uint64_t)in[9] << 32), out);)
OP(StreamU32, 10, CHK_U32 + 2, RngStream s(rng_state_from_words(in)); for (int i = 0; i < CHK_U32; i++) out[i] = s.next_u32(); st_pos(out + CHK_U32, s.st.word_pos);)
OP(StreamU64, 10, 2 * CHK_U64 + 2, RngStream s(rng_state_from_words(in));
   for (int i = 0; i < CHK_U64; i++) { const uint64_t v = rng_next_u64(s); out[2 * i] = (uint32_t)v; out[2 * i + 1] = (uint32_t)(v >> 32); }
   st_pos(out + 2 * CHK_U64, s.st.word_pos);)
OP(FrRand, 10, 8 * CHK_FR + 2, RngStream s(rng_state_from_words(in)); for (int i = 0; i < CHK_FR; i++) rng_fr(s, out + 8 * i); st_pos(out + 8 * CHK_FR, s.st.word_pos);)
OP(FrAccept, 8, 9, uint32_t l[8]; for (int i = 0; i < 8; i++) l[i] = in[i]; out[8] = rng_fr_accept(l) ? 1u : 0u; for (int i = 0; i < 8; i++) out[i] = l[i];)
OP(RangeAccept, 2, 3, uint32_t hi; out[0] = rng_range_zone(in[1]); out[2] = rng_range_accept(in[0], in[1], out[0], hi) ? 1u : 0u; out[1] = hi;)
OP(GenRange, 11, 3, RngStream s(rng_state_from_words(in)); out[0] = rng_gen_range(s, in[10]); st_pos(out + 1, s.st.word_pos);)
// a shuffle of 0..len, len <= CHK_SHUFFLE (longer: clamped); the unused tail stays the identity
OP(Shuffle, 11, CHK_SHUFFLE + 2, RngStream s(rng_state_from_words(in)); for (int i = 0; i < CHK_SHUFFLE; i++) out[i] = (uint32_t)i;
   rng_shuffle(s, out, in[10] < (uint32_t)CHK_SHUFFLE ? in[10] : (uint32_t)CHK_SHUFFLE); st_pos(out + CHK_SHUFFLE, s.st.word_pos);)
OP(SeedFromU64, 2, 10, rng_state_to_words(rng_seed_from_u64((uint64_t)in[0] | ((uint64_t)in[1] << 32)), out);)
OP(Split, 10, 12, RngStream s(rng_state_from_words(in)); rng_state_to_words(rng_split(s), out); st_pos(out + 10, s.st.word_pos);)
OP(PosValid, 2, 1, out[0] = rng_pos_valid((uint64_t)in[0] | ((uint64_t)in[1] << 32)) ? 1u : 0u;)

static const Entry TABLE[] = {
    entry<Block>("chacha12_block"), entry<StreamU32>("next_u32"), entry<StreamU64>("next_u64"), entry<FrRand>("fr_rand"), entry<FrAccept>("fr_accept"),
    entry<RangeAccept>("range_accept"), entry<GenRange>("gen_range"), entry<Shuffle>("shuffle"), entry<SeedFromU64>("seed_from_u64"), entry<Split>("split"),
    entry<PosValid>("pos_valid"),
};

int main(int argc, char** argv) { return rows_main(argc, argv, TABLE); }
