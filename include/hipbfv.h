/*
 * include/hipbfv.h -- C ABI of libhipbfv.so, the MI355X-native BFV ciphertext-arithmetic backend.
 *
 * This is the drop-in boundary for the one hot path of the reference: everything that
 * `seal_fhe::Evaluator` (seal_fhe/src/evaluator.rs:7-280) forwards to Microsoft SEAL's C API
 * through bindgen.  Part 1 re-exports the SEAL C entry points that the `seal_fhe` crate binds for
 * that path, with the same names, argument order, opaque `void*` handles and HRESULT return values,
 * so that the files under `seal_fhe/src/` can link against this library unchanged.
 * Part 2 is the extension the reference API lacks: raw-array import/export for handles and the
 * batched, device-pointer entry points used by the GPU batch executor.
 *
 * Conventions (seal_fhe/src/lib.rs:28-34, error.rs:65-91):
 *   - every function returns a `long` HRESULT: S_OK = 0 on success;
 *   - objects are opaque `void*` created through an out-parameter and destroyed by X_Destroy;
 *   - `pool` arguments are accepted and ignored (the crate always passes NULL);
 *   - in-place calls alias `destination` with an operand (evaluator_base.rs:107-113,184-196);
 *   - all handle-level calls are synchronous and may be issued concurrently from several host
 *     threads on one evaluator handle (sunscreen_runtime/src/run.rs:415-469).
 * Ciphertext data layout: u64[size][K][N], K = data-level primes, N = poly degree
 * (seal_fhe/src/plaintext_ciphertext.rs:303-314).  Key-switching key: u64[K][2][K+1][N], NTT form.
 */
#ifndef HIPBFV_H
#define HIPBFV_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPBFV_S_OK 0L
#define HIPBFV_E_POINTER ((long)0x80004003L)
#define HIPBFV_E_INVALIDARG ((long)0x80070057L)
#define HIPBFV_E_OUTOFMEMORY ((long)0x8007000EL)
#define HIPBFV_E_UNEXPECTED ((long)0x8000FFFFL)
#define HIPBFV_COR_E_IO ((long)0x80131620L)
#define HIPBFV_COR_E_INVALIDOPERATION ((long)0x80131509L)

/* ===================================================================================== */
/* Part 1: SEAL C API subset bound by seal_fhe for the evaluator path                      */
/* ===================================================================================== */

/* ---- Modulus (seal_fhe/src/modulus.rs:225-262) ---- */
long Modulus_Create1(uint64_t value, void **small_modulus);
long Modulus_Create2(void *copy, void **small_modulus);
long Modulus_Destroy(void *thisptr);
long Modulus_Value(void *thisptr, uint64_t *result);

/* ---- CoeffModulus helpers (seal_fhe/src/modulus.rs:149-205) ---- */
long CoeffModulus_MaxBitCount(uint64_t poly_modulus_degree, int sec_level, int *bit_count);
long CoeffModulus_BFVDefault(uint64_t poly_modulus_degree, int sec_level, uint64_t *length, void **coeffs);
long CoeffModulus_Create1(uint64_t poly_modulus_degree, uint64_t length, int *bit_sizes, void **coeffs);
/* PlainModulus::batching is CoeffModulus_Create1 with one entry (seal_fhe/src/modulus.rs:100-116) */

/* ---- EncryptionParameters (seal_fhe/src/encryption_parameters.rs:100-330); scheme 1 = BFV ---- */
long EncParams_Create1(uint8_t scheme, void **enc_params);
long EncParams_Destroy(void *thisptr);
long EncParams_SetPolyModulusDegree(void *thisptr, uint64_t degree);
long EncParams_GetPolyModulusDegree(void *thisptr, uint64_t *degree);
long EncParams_SetCoeffModulus(void *thisptr, uint64_t length, void **coeffs);
long EncParams_GetCoeffModulus(void *thisptr, uint64_t *length, void **coeffs);
long EncParams_SetPlainModulus1(void *thisptr, void *modulus);
long EncParams_SetPlainModulus2(void *thisptr, uint64_t plain_modulus);
long EncParams_GetPlainModulus(void *thisptr, void **plain_modulus);
long EncParams_GetScheme(void *thisptr, uint8_t *scheme);

/* ---- SEALContext (seal_fhe/src/context.rs:63-115); sec_level: 0 none, 128, 192, 256 ---- */
long SEALContext_Create(void *encryption_params, bool expand_mod_chain, int sec_level, void **context);
long SEALContext_Destroy(void *thisptr);

/* ---- Plaintext (seal_fhe/src/plaintext_ciphertext.rs:36-300) ---- */
long Plaintext_Create1(void *pool, void **plaintext);
long Plaintext_Create4(char *hex_poly, void *pool, void **plaintext); /* "7FFx^3 + 1x^1 + 3", plaintext_ciphertext.rs:180-217 */
long Plaintext_Create5(void *copy, void **plaintext);
long Plaintext_Destroy(void *thisptr);
long Plaintext_CoeffCount(void *thisptr, uint64_t *coeff_count);
long Plaintext_CoeffAt(void *thisptr, uint64_t index, uint64_t *coeff);
long Plaintext_SetCoeffAt(void *thisptr, uint64_t index, uint64_t value);
long Plaintext_Resize(void *thisptr, uint64_t coeff_count);
long Plaintext_IsNTTForm(void *thisptr, bool *is_ntt_form);
/* SEAL 4.0 wire format; compr_mode 0 = none, 2 = zstd (seal_fhe/src/plaintext_ciphertext.rs:100-160) */
long Plaintext_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result);
long Plaintext_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes);
long Plaintext_Load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);

/* ---- Ciphertext (seal_fhe/src/plaintext_ciphertext.rs:326-504) ---- */
long Ciphertext_Create1(void *pool, void **cipher);
long Ciphertext_Create2(void *copy, void **cipher);
long Ciphertext_Destroy(void *thisptr);
long Ciphertext_Size(void *thisptr, uint64_t *size);
long Ciphertext_CoeffModulusSize(void *thisptr, uint64_t *coeff_modulus_size);
long Ciphertext_PolyModulusDegree(void *thisptr, uint64_t *poly_modulus_degree);
long Ciphertext_GetDataAt1(void *thisptr, uint64_t index, uint64_t *data);
long Ciphertext_GetDataAt2(void *thisptr, uint64_t poly_index, uint64_t coeff_index, uint64_t *data);
long Ciphertext_IsNTTForm(void *thisptr, bool *is_ntt_form);
/* SEAL 4.0 wire format (seal_fhe/src/plaintext_ciphertext.rs:451-497) */
long Ciphertext_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result);
long Ciphertext_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes);
long Ciphertext_Load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);

/* ---- KSwitchKeys: RelinKeys and GaloisKeys (seal_fhe/src/key_generator.rs:467-729) ---- */
long KSwitchKeys_Create1(void **kswitch_keys);
long KSwitchKeys_Create2(void *copy, void **kswitch_keys);
long KSwitchKeys_Destroy(void *thisptr);
/* SEAL 4.0 wire format (seal_fhe/src/key_generator.rs:493-573, 649-729) */
long KSwitchKeys_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result);
long KSwitchKeys_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes);
long KSwitchKeys_Load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);

/* ---- SecretKey / PublicKey (seal_fhe/src/key_generator.rs:200-430): handles + SEAL 4.0 wire format.
 * Key data is key-level NTT form:
 * SecretKey u64[K+1][N], PublicKey u64[2][K+1][N]. ---- */
long SecretKey_Create1(void **key);
long SecretKey_Create2(void *copy, void **key);
long SecretKey_Destroy(void *thisptr);
long SecretKey_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result);
long SecretKey_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes);
long SecretKey_Load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);
long PublicKey_Create1(void **key);
long PublicKey_Create2(void *copy, void **key);
long PublicKey_Destroy(void *thisptr);
long PublicKey_SaveSize(void *thisptr, uint8_t compr_mode, int64_t *result);
long PublicKey_Save(void *thisptr, uint8_t *outptr, uint64_t size, uint8_t compr_mode, int64_t *out_bytes);
long PublicKey_Load(void *thisptr, void *context, uint8_t *inptr, uint64_t size, int64_t *in_bytes);

/* ---- KeyGenerator (seal_fhe/src/key_generator.rs:20-200): keys are sampled and assembled on the device (Philox4x32-10;
 * ternary secret, uniform a, rounded Gaussian errors; key-switching keys in SEAL's layout u64[K][2][K+1][N]).  Like
 * SEAL's, the keys are not reproducible across implementations; they interoperate through the wire format.
 * save_seed (seed-compressed serialisation) is accepted and ignored: handles always hold expanded keys. ---- */
long KeyGenerator_Create1(void *context, void **key_generator);
long KeyGenerator_Create2(void *context, void *secret_key, void **key_generator);
long KeyGenerator_Destroy(void *thisptr);
long KeyGenerator_SecretKey(void *thisptr, void **secret_key);
long KeyGenerator_CreatePublicKey(void *thisptr, bool save_seed, void **public_key);
long KeyGenerator_CreateRelinKeys(void *thisptr, bool save_seed, void **relin_keys);
long KeyGenerator_CreateGaloisKeysFromElts(void *thisptr, uint64_t count, uint32_t *galois_elts, bool save_seed, void **galois_keys);
long KeyGenerator_CreateGaloisKeysAll(void *thisptr, bool save_seed, void **galois_keys);
long KeyGenerator_CreateGaloisKeysFromSteps(void *thisptr, uint64_t count, int *steps, bool save_seed, void **galois_keys); /* SEAL keygenerator.h; not bound by seal_fhe */

/* ---- BatchEncoder (seal_fhe/src/encoder.rs:50-215): slot vectors <-> plaintexts, transforms over Z_t on the device ---- */
long BatchEncoder_Create(void *context, void **encoder);
long BatchEncoder_Destroy(void *thisptr);
long BatchEncoder_Encode1(void *thisptr, uint64_t count, uint64_t *values, void *destination);
long BatchEncoder_Encode2(void *thisptr, uint64_t count, int64_t *values, void *destination);
long BatchEncoder_Decode1(void *thisptr, void *plain, uint64_t *count, uint64_t *destination, void *pool);
long BatchEncoder_Decode2(void *thisptr, void *plain, uint64_t *count, int64_t *destination, void *pool);
long BatchEncoder_GetSlotCount(void *thisptr, uint64_t *slot_count);

/* ---- Decryptor (seal_fhe/src/encryptor_decryptor.rs:596-690): <ct, (1, s, s^2)> then SEAL's
 * decrypt_scale_and_round in the base {t, gamma}; bit-identical plaintexts ---- */
long Decryptor_Create(void *context, void *secret_key, void **decryptor);
long Decryptor_Destroy(void *thisptr);
long Decryptor_Decrypt(void *thisptr, void *encrypted, void *destination);
long Decryptor_InvariantNoiseBudget(void *thisptr, void *encrypted, int *invariant_noise_budget);
long Decryptor_InvariantNoise(void *thisptr, void *encrypted, double *invariant_noise); /* fork: encryptor_decryptor.rs:660-683 */

/* ---- Encryptor (seal_fhe/src/encryptor_decryptor.rs:140-600).  The randomness is the library's own (Philox4x32-10;
 * ternary u, rounded Gaussian sigma 3.2 clipped at 19, uniform a): ciphertexts are valid SEAL ciphertexts but, like
 * SEAL's, not reproducible across implementations.  public_key or secret_key may be NULL (with_public_key /
 * with_secret_key / with_public_and_secret_key).  The *ReturnComponents* entry points are the Sunscreen fork's
 * (encryptor_decryptor.rs:268-590): they also hand back the sampled u (1 polynomial), e (2; 1 in symmetric mode) as
 * PolynomialArrays over the data primes and the scaling remainder r, such that over the data primes, exactly,
 *   public key, disable_special_modulus: c0 = floor(q/t) m + r + pk0 u + e0,  c1 = pk1 u + e1
 *   secret key:                          c0 = floor(q/t) m + r - (c1 s + e)
 * (logproof/src/bfv_statement.rs:159-160).  The *SetSeed variants take the fork's [u64; 8] seed, folded into the
 * Philox key: equal seeds give equal ciphertexts (not SEAL's bits: its PRNG is not restated).  save_seed is ignored. ---- */
long Encryptor_Create(void *context, void *public_key, void *secret_key, void **encryptor);
long Encryptor_Destroy(void *thisptr);
long Encryptor_Encrypt(void *thisptr, void *plaintext, void *destination, void *pool);
long Encryptor_EncryptReturnComponents(void *thisptr, void *plaintext, bool disable_special_modulus, void *destination,
                                       void *u_destination, void *e_destination, void *r_destination, void *pool);
long Encryptor_EncryptReturnComponentsSetSeed(void *thisptr, void *plaintext, bool disable_special_modulus, void *destination,
                                              void *u_destination, void *e_destination, void *r_destination, void *seed, void *pool);
long Encryptor_EncryptSymmetric(void *thisptr, void *plaintext, bool save_seed, void *destination, void *pool);
long Encryptor_EncryptSymmetricReturnComponents(void *thisptr, void *plaintext, void *destination, void *e_destination,
                                                void *r_destination, void *pool);
long Encryptor_EncryptSymmetricReturnComponentsSetSeed(void *thisptr, void *plaintext, void *destination, void *e_destination,
                                                       void *r_destination, void *seed, void *pool);

/* ---- PolynomialArray, the Sunscreen fork's export type (seal_fhe/src/data_structures.rs:17-304): `PolySize`
 * coefficient-form polynomials over the first `CoeffModulusSize` primes, exported either as RNS u64[poly][rns][coeff]
 * or, after ToMultiprecision, as u64[poly][coeff][limb] (CRT-composed value in [0, q), little-endian limbs) -- the layout
 * logproof/src/bfv_statement.rs:624-660 consumes.  Keys are converted out of NTT form and restricted to the data primes.
 * The conversions run on the device.  Drop keeps residues 0..k-2 of every polynomial. ---- */
long PolynomialArray_Create(void *pool, void **poly_array);
long PolynomialArray_CreateFromCiphertext(void *pool, void *context, void *ciphertext, void **poly_array);
long PolynomialArray_CreateFromPublicKey(void *pool, void *context, void *public_key, void **poly_array);
long PolynomialArray_CreateFromSecretKey(void *pool, void *context, void *secret_key, void **poly_array);
long PolynomialArray_Copy(void *copy, void **poly_array);
long PolynomialArray_Destroy(void *thisptr);
long PolynomialArray_IsReserved(void *thisptr, bool *is_reserved);
long PolynomialArray_IsRns(void *thisptr, bool *is_rns);
long PolynomialArray_ToRns(void *thisptr);
long PolynomialArray_ToMultiprecision(void *thisptr);
long PolynomialArray_PolySize(void *thisptr, uint64_t *size);
long PolynomialArray_PolyModulusDegree(void *thisptr, uint64_t *size);
long PolynomialArray_CoeffModulusSize(void *thisptr, uint64_t *size);
long PolynomialArray_ExportSize(void *thisptr, uint64_t *size);
long PolynomialArray_PerformExport(void *thisptr, uint64_t *data);
long PolynomialArray_Drop(void *thisptr, void **poly_array);

/* ---- Evaluator (seal_fhe/src/evaluator_base.rs:55-407, bfv_evaluator.rs:12-248) ---- */
long Evaluator_Create(void *seal_context, void **evaluator);
long Evaluator_Destroy(void *thisptr);
long Evaluator_Negate(void *thisptr, void *encrypted, void *destination);
long Evaluator_Add(void *thisptr, void *encrypted1, void *encrypted2, void *destination);
long Evaluator_AddMany(void *thisptr, uint64_t count, void **encrypteds, void *destination);
long Evaluator_Sub(void *thisptr, void *encrypted1, void *encrypted2, void *destination);
long Evaluator_Multiply(void *thisptr, void *encrypted1, void *encrypted2, void *destination, void *pool);
long Evaluator_MultiplyMany(void *thisptr, uint64_t count, void **encrypteds, void *relin_keys, void *destination, void *pool);
/* Square = Multiply(x, x) bit for bit; when the two operands of a multiply are ONE ciphertext (here, Evaluator_Multiply with
 * encrypted1 == encrypted2, hipbfv_batch_multiply* with a == b, a program node whose operands are one node) the kernels extend
 * and transform it once: two forward transforms per residue instead of four. */
long Evaluator_Square(void *thisptr, void *encrypted, void *destination, void *pool);
long Evaluator_Relinearize(void *thisptr, void *encrypted, void *relin_keys, void *destination, void *pool);
long Evaluator_Exponentiate(void *thisptr, void *encrypted, uint64_t exponent, void *relin_keys, void *destination, void *pool);
long Evaluator_AddPlain(void *thisptr, void *encrypted, void *plain, void *destination);
long Evaluator_SubPlain(void *thisptr, void *encrypted, void *plain, void *destination);
long Evaluator_MultiplyPlain(void *thisptr, void *encrypted, void *plain, void *destination, void *pool);
long Evaluator_RotateRows(void *thisptr, void *encrypted, int steps, void *galois_keys, void *destination, void *pool);
long Evaluator_RotateColumns(void *thisptr, void *encrypted, void *galois_keys, void *destination, void *pool);
/* mod_switch_to_next (seal_fhe/src/evaluator.rs:84-157): BFV ciphertexts are divided-and-rounded by the last data prime
 * and move to the next level of the modulus-switching chain; every Evaluator_*, Decryptor_* and Ciphertext_Save/Load
 * call accepts ciphertexts of any level (levels are created on first use; SEALContext_Create(expand_mod_chain = false)
 * disables them).  Plaintexts of this path are never in NTT form, so the plaintext overload always fails as SEAL's does. */
long Evaluator_ModSwitchToNext1(void *thisptr, void *encrypted, void *destination, void *pool);
long Evaluator_ModSwitchToNext2(void *thisptr, void *plain, void *destination);

/* ===================================================================================== */
/* Part 2: hipbfv extensions                                                               */
/* ===================================================================================== */

/* Library / device */
long hipbfv_version(uint32_t *major, uint32_t *minor);
long hipbfv_last_error(char *buffer, uint64_t capacity);       /* thread-local message of the last failure */
long hipbfv_build_flags(char *buffer, uint64_t capacity);      /* compiler flags (-D set included) this library was built with */
long hipbfv_set_device(int device);                            /* HIP device used by contexts created afterwards */
/* SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT switch (seal_fhe `transparent-ciphertexts` feature): default on */
long hipbfv_set_throw_on_transparent(bool enabled);

/* Context shortcuts: build a context straight from raw parameters.
 * Accepted: poly_modulus_degree a power of two in [1024, 32768]; distinct primes below 2^60, each == 1 mod 2n; a plain modulus t
 * in [2, 2^60) that shares no factor with the data primes (SEAL's bit-count and coprimality rules).  Every such t is supported,
 * batching or not, odd or a power of two, above a data prime or not.  Anything else fails with E_INVALIDARG (the oracle model
 * does not check t; tests/test_gpu_plain_modulus.py checks the refusals). */
long hipbfv_Context_Create(uint64_t poly_modulus_degree, const uint64_t *coeff_modulus, uint64_t coeff_count,
                           uint64_t plain_modulus, void **context);
long hipbfv_Context_Info(void *context, uint64_t *poly_modulus_degree, uint64_t *data_primes, uint64_t *key_primes,
                         uint64_t *plain_modulus);
long hipbfv_Context_GetPrime(void *context, uint64_t index, uint64_t *value); /* key-level prime `index` */
/* the context of the next level of the modulus-switching chain (one data prime fewer, same special prime): an owned
 * handle for the batched API (Evaluator_Create on it, hipbfv_batch_* at that level) */
long hipbfv_Context_NextLevel(void *context, void **next);
/* The BEHZ auxiliary base Bsk = B u {m_sk} this context multiplies in (internal to Evaluator_Multiply; SEAL's
 * RNSTool keeps its own privately, native/src/seal/util/rns.h).  *fp64_base bit 0 = the library chose its own
 * FP64-pipe primes (same size bound as SEAL's rule, bit-identical products) instead of SEAL's 61-bit primes;
 * bit 1 / bit 2 = the split multiply / key-switch pipelines store their intermediates 48-bit packed; bit 3 = the
 * multiply forms its q -> Bsk base-conversion sums exactly and reduces each once; bit 4 = mixed base: the data primes are too
 * wide for the FP64 pipe (the 3 x 54-bit set) but the auxiliary primes are the library's own FP64-pipe ones; bit 5 = the multiply packs
 * its intermediates PER ROW: only the rows whose prime is below 2^48 (the SEAL default set of n = 16384: 13 of 18 rows); bit 6 = the key
 * switch packs its digit rows per KEY PRIME (bit 2 is set too; n = 16384: the rows of 3 of the 9 key primes) (diagnostics).
 * primes may be NULL; otherwise capacity >= *count words, B first, m_sk last. */
long hipbfv_Context_AuxBase(void *context, uint64_t *count, uint64_t *primes, uint64_t capacity, int *fp64_base);

/* Raw-array import/export for handles (host memory): the no-serialisation alternative to X_Load / X_Save */
long hipbfv_Ciphertext_Assign(void *cipher, void *context, uint64_t size, const uint64_t *host_data);
long hipbfv_Ciphertext_Export(void *cipher, uint64_t *host_data, uint64_t capacity_words);
long hipbfv_Ciphertext_DevicePtr(void *cipher, uint64_t **device_ptr);
long hipbfv_KSwitchKeys_AssignRelin(void *keys, void *context, const uint64_t *host_data);
long hipbfv_KSwitchKeys_AssignGalois(void *keys, void *context, uint32_t galois_elt, const uint64_t *host_data);
long hipbfv_KSwitchKeys_DevicePtr(void *keys, uint64_t index, uint64_t **device_ptr); /* index 0 = relin, (elt-1)/2 = galois */
long hipbfv_KSwitchKeys_Read(void *keys, uint64_t index, uint64_t *host_out);          /* u64[K][2][K+1][N] */
long hipbfv_KSwitchKeys_Has(void *keys, uint64_t index, bool *present);
long hipbfv_SecretKey_Read(void *key, uint64_t *host_out);                              /* u64[K+1][N] */
long hipbfv_PublicKey_Read(void *key, uint64_t *host_out);                              /* u64[2][K+1][N] */
long hipbfv_SecretKey_Assign(void *key, void *context, const uint64_t *host_data);  /* u64[K+1][N], NTT form */
long hipbfv_PublicKey_Assign(void *key, void *context, const uint64_t *host_data);  /* u64[2][K+1][N], NTT form */
long hipbfv_Encryptor_SetSeed(void *encryptor, uint64_t seed);                      /* reproducible runs (tests) */
long hipbfv_KeyGenerator_SetSeed(void *key_generator, uint64_t seed);               /* keys created afterwards */
long hipbfv_KeyGenerator_CreateSeeded(void *context, uint64_t seed, void **key_generator); /* reproducible secret */
/* TEST ONLY: sigma_g(secret) in coefficient form, u64[K+1][N], as the Galois key of galois_elt takes it up before its
 * forward transform (every word canonical: a sign-flipped 0 is 0) */
long hipbfv_debug_keygen_galois_secret(void *key_generator, uint32_t galois_elt, uint64_t *host_out);

/* Host-only helpers of the SEAL 4.0 wire format (no device access; used by the CPU tests against the
 * reference's binary fixtures): parms_id = BLAKE2b-256([scheme=1, n, primes..., t]); decode/encode one object. */
long hipbfv_wire_parms_id(uint64_t poly_modulus_degree, const uint64_t *primes, uint64_t count, uint64_t plain_modulus,
                          uint8_t *out32);
long hipbfv_wire_decode_ciphertext(const uint8_t *in, uint64_t in_size, uint8_t *parms_id32, bool *is_ntt, uint64_t *size,
                                   uint64_t *poly_modulus_degree, uint64_t *coeff_modulus_size, uint64_t *data,
                                   uint64_t capacity_words, int64_t *in_bytes);
long hipbfv_wire_encode_ciphertext(const uint8_t *parms_id32, bool is_ntt, uint64_t size, uint64_t poly_modulus_degree,
                                   uint64_t coeff_modulus_size, const uint64_t *data, uint8_t compr_mode, uint8_t *out,
                                   uint64_t capacity, int64_t *out_bytes);
long hipbfv_wire_decode_plaintext(const uint8_t *in, uint64_t in_size, uint8_t *parms_id32, uint64_t *coeff_count,
                                  uint64_t *coeffs, uint64_t capacity_words, int64_t *in_bytes);

/* Batched entry points: device pointers, `count` independent ciphertexts u64[count][size][K][N],
 * enqueued asynchronously on `stream` (a hipStream_t; NULL = default stream).
 *
 * Aliasing.  An output may be EXACTLY one of the inputs (the same pointer) when it has the same number of words per item as
 * that input: add(a, b, out = a), multiply_relin(a, a, out = a), rotate_rows(ct, steps, out = ct) and the like.  Any other
 * overlap between an output range and any input range is HIPBFV_E_INVALIDARG, and nothing is launched.  The ranges are
 * [ptr, ptr + count * words_per_item) (a plaintext operand: its plaintext width, one item when shared).  So the calls whose
 * output is wider or narrower than their input (multiply 2 + 2 -> 3 polynomials, relinearize 3 -> 2, mod_switch K -> K-1) take
 * no in-place form, and an output shifted against its input by any amount is refused.  The transforms either side of the
 * evaluator (encode, decode, decrypt, encrypt, plain_to_ntt, ct_to_ntt, dot_plain_ntt,
 * dot_plain_ntt_queries) accept no overlap at all.  So do the
 * noise measures (noise_budget, decrypt_checked): no output may overlap `ct`, and no output may overlap another output (byte
 * ranges: budget is int32_t[count], noise double[count]); any overlap is HIPBFV_E_INVALIDARG before anything is launched.
 * hipbfv_batch_ntt works in place by definition. */
long hipbfv_batch_multiply(void *evaluator, const uint64_t *a, uint64_t size_a, const uint64_t *b, uint64_t size_b,
                           uint64_t *out, uint64_t count, void *stream);
long hipbfv_batch_relinearize(void *evaluator, const uint64_t *ct3, void *relin_keys, uint64_t *out2, uint64_t count,
                              void *stream);
long hipbfv_batch_multiply_relin(void *evaluator, const uint64_t *a, const uint64_t *b, void *relin_keys,
                                 uint64_t *out2, uint64_t count, void *stream);
long hipbfv_batch_apply_galois(void *evaluator, const uint64_t *ct2, uint32_t galois_elt, void *galois_keys,
                               uint64_t *out2, uint64_t count, void *stream);
/* Row rotations, here and in every other entry point that takes `steps` (Evaluator_RotateRows, the *_keys, *_items and pool
 * forms, a program's rotation nodes), decide as SEAL's rotate_internal does: step 0 copies; the step's own Galois key when the
 * key set holds it; otherwise the power-of-two keys of the step's non-adjacent form (NAF), least significant part first, the
 * part of N/2 rows left out.  The whole decision is made on the host before the first launch: a refused rotation
 * (|steps| >= N/2, or neither the step's own key nor every key of its chain) launches nothing and leaves a destination that is
 * not the input as it was. */
long hipbfv_batch_rotate_rows(void *evaluator, const uint64_t *ct2, int steps, void *galois_keys, uint64_t *out2,
                              uint64_t count, void *stream);
long hipbfv_batch_rotate_columns(void *evaluator, const uint64_t *ct2, void *galois_keys, uint64_t *out2,
                                 uint64_t count, void *stream);
/* Mixed-step rotation batches: item i by its OWN Galois element / step (a server that batches many clients' rotations, the
 * diagonals of a matrix-vector product, the baby and giant steps of a sum), one key set for the call.  galois_elts / steps are
 * HOST arrays of `count` entries, read before the call returns.
 *  - apply_galois_items: every element odd and below 2 N; element 1 copies the item; every other element's key must be held.
 *  - rotate_rows_items: item i has exactly the bits of hipbfv_batch_rotate_rows called with steps[i] on that item alone, so
 *    every distinct step decides as SEAL's rotate_internal does: step 0 copies, a step whose element's key is held rotates
 *    through it, any other step runs its NAF chain of power-of-two keys (together with the other items of that step).
 * All the items that rotate through a key of their own share ONE key-switch launch sequence: the kernels take the automorphism
 * and the key per item, and walk the items in element order, so that an element's key rows are shared in one XCD's L2.  Items
 * need not be grouped by step.  A refused element or step (|step| >= N/2) and a missing key (a chain's included) fail the
 * whole call with HIPBFV_E_INVALIDARG before anything is launched or written; hipbfv_last_error names the first such item
 * ("item <index>: ...").  Aliasing as above: out2 may be exactly ct2, any other overlap is refused. */
long hipbfv_batch_apply_galois_items(void *evaluator, const uint64_t *ct2, const uint32_t *galois_elts, void *galois_keys,
                                     uint64_t *out2, uint64_t count, void *stream);
long hipbfv_batch_rotate_rows_items(void *evaluator, const uint64_t *ct2, const int32_t *steps, void *galois_keys,
                                    uint64_t *out2, uint64_t count, void *stream);
/* Sums of rotations: out2[g] = sum_t rotate_rows(source of item g * terms + t, steps[t]) -- the giant-step sum of a baby-step /
 * giant-step matrix-vector product, a moving-window or prefix sum over slots, a convolution with a few taps, a replicated slot --
 * with every term finished and added inside the key switch's last kernel: a term's rows are never written and no add pass runs.
 *  - Layouts: ct2 device u64[sources][2][K][N]; out2 device u64[groups][2][K][N]; steps / galois_elts HOST arrays of `terms`
 *    entries, shared by every group (as `weights` in hipbfv_batch_multiply_sum_weighted); src_index a HOST array of index_len
 *    entries; all host arrays are read before the call returns.  Item i = g * terms + t reads source src_index[i % index_len];
 *    src_index == NULL means source i, and then sources must equal groups * terms.  (NULL: a sum of distinct ciphertexts;
 *    src_index[i] = i / terms with index_len = groups * terms: one ciphertext per group by many steps; {0, ..., terms - 1}: one set
 *    of ciphertexts shared by all groups.)  Nothing is replicated in memory.
 *  - Bits: out2[g] is, word for word, the sum (hipbfv_batch_add, in any order) of hipbfv_batch_rotate_rows(source, steps[t]) over the
 *    group's terms -- of hipbfv_batch_apply_galois for the Galois form.  Every distinct step decides as SEAL's rotate_internal does:
 *    step 0 (element 1) contributes the source itself, a step whose element's key is held rotates through it, any other step
 *    walks its NAF chain.  With terms == 1 the result equals hipbfv_batch_rotate_rows_items (hipbfv_batch_apply_galois_items).  The
 *    same (source, step) listed twice contributes twice.  Neither one decomposition shared by many steps nor one mod-down shared by
 *    a group's terms would give these bits: every term runs its own key switch up to its own mod-down.
 *  - Refusals, all before anything is launched, copied or written: a NULL evaluator, ct2, out2, steps (galois_elts) or key object
 *    is HIPBFV_E_POINTER; HIPBFV_E_INVALIDARG: terms == 0; src_index != NULL with index_len == 0; an index >= sources; src_index
 *    == NULL with sources != groups * terms; |step| >= N/2, or an even or too large element; a missing direct key or chain key; ANY
 *    overlap of the out2 range with the ct2 range (there is no in-place form: a group's sum would be written while other groups
 *    still read their sources); more than 2^32 - 1 groups or terms.  groups == 0 returns HIPBFV_S_OK, nothing launched.  Parameters
 *    without batching give the row form HIPBFV_COR_E_INVALIDOPERATION.  hipbfv_last_error names the first offender: "term <t>: ..."
 *    for a step, an element or a key, "item <i>: ..." for an index.
 *  - Launches: where the key switch takes the split kernels for groups * terms items (N = 4096 ... 16384), a chunk is a whole
 *    number of groups and runs ONE head / middle / summing-tail sequence for all its direct-key and identity terms; a group with
 *    more terms than a chunk holds is summed in slices (hipbfv_debug_rotate_sum_plan).  Chain terms are rotated beforehand by the
 *    chain of hipbfv_batch_rotate_rows into a staging buffer -- each distinct (source, step) once -- and enter the sum as identity
 *    terms.  Elsewhere (N < 4096, N = 32768, a few items, HIPBFV_NO_FUSED_GALOIS=1) the terms are rotated into a staging buffer and
 *    folded by the element-wise add: the same bits.  Asynchronous on `stream`.
 *  - Transparent results: the sums are recorded under GROUP numbers (hipbfv_batch_status); a transparent term inside a sum that is
 *    not transparent is NOT detected. */
long hipbfv_batch_rotate_rows_sum(void *evaluator, const uint64_t *ct2, uint64_t sources, const uint32_t *src_index,
                                  uint64_t index_len, const int32_t *steps, void *galois_keys, uint64_t *out2, uint64_t groups,
                                  uint64_t terms, void *stream);
long hipbfv_batch_apply_galois_sum(void *evaluator, const uint64_t *ct2, uint64_t sources, const uint32_t *src_index,
                                   uint64_t index_len, const uint32_t *galois_elts, void *galois_keys, uint64_t *out2,
                                   uint64_t groups, uint64_t terms, void *stream);
/* Weighted sums of rotations: out2[g] = sum_t w_t (.) rotate_rows(source of item g * terms + t, steps[t]) -- a convolution or FIR
 * filter with taps (1, -2, 1), a finite difference x - rotate(x, 1), a weighted moving window, the signed giant-step sum of a baby-step
 * / giant-step product -- with the weight applied to every finished term inside the key switch's last kernel, just before it is added.
 * (.) is hipbfv_batch_multiply_sum_weighted's: every word of residue row i of the finished term is multiplied by (w_t mod q_i), taken
 * canonically in [0, q_i), mod q_i -- the words of |w| hipbfv_batch_add calls of the rotated ciphertext, after hipbfv_batch_negate
 * when w < 0.  No transform pair, no plaintext; a weight multiplies its term's noise by |w|.
 *  - weights: a HOST array of `terms` int32_t, shared by every group as `steps` is, read before the call returns.  Any int32_t is a
 *    weight, 0, -1, INT32_MIN and INT32_MAX included.  A zero weight is a weight like any other: its term is planned, validated,
 *    refused and launched as any other term.
 *  - Everything hipbfv_batch_rotate_rows_sum (hipbfv_batch_apply_galois_sum) promises carries over: layouts, src_index, every refusal
 *    before anything is launched, copied or written, no in-place form, chunks and slices, transparent results under GROUP numbers.
 *    In addition a NULL `weights` is HIPBFV_E_POINTER.
 *  - A table of all ones is not staged and runs the unweighted launches: the same words and the same profiler counts.  All weights
 *    0, or (+1, -1) on the same (source, step), give a transparent sum, reported under its group number.  The same (source, step)
 *    listed twice with weights w1 and w2 contributes (w1 + w2).
 *  - Launches: the unweighted call's, with the weighted sibling of the summing tail (same profiler kind, same units); chain terms
 *    stay deduplicated per distinct (source, step) and are weighted where they enter the sum.  Off the split path the staged terms
 *    are folded by one scaled accumulate per term and group (out = (out or 0) + w * x): the same bits. */
long hipbfv_batch_rotate_rows_sum_weighted(void *evaluator, const uint64_t *ct2, uint64_t sources, const uint32_t *src_index,
                                           uint64_t index_len, const int32_t *steps, const int32_t *weights, void *galois_keys,
                                           uint64_t *out2, uint64_t groups, uint64_t terms, void *stream);
long hipbfv_batch_apply_galois_sum_weighted(void *evaluator, const uint64_t *ct2, uint64_t sources, const uint32_t *src_index,
                                            uint64_t index_len, const uint32_t *galois_elts, const int32_t *weights,
                                            void *galois_keys, uint64_t *out2, uint64_t groups, uint64_t terms, void *stream);
/* Per-key batches (multi-tenant serving).  The reference hands the keys over with every call
 * (sunscreen_runtime/src/run.rs:100-105: `relin_keys: &Option<&RelinearizationKeys>`, `galois_keys: &Option<&GaloisKeys>`;
 * runtime.rs:310-327), so a server that batches the calls of many clients holds one key set per client.  These are the
 * three key-switching operations above with `num_key_sets` key handles (RelinearizationKeys resp. GaloisKeys objects of the
 * evaluator's context) and, per item, the set it uses: key_index is a HOST array of `count` entries < num_key_sets, read
 * before the call returns.  Item i gives the bits of the single-key call with key_sets[key_index[i]], whoever else is in the
 * batch.  Only the REFERENCED sets (those key_index names) are validated and read: an unreferenced entry may be NULL, a set
 * without the key or a key object of another context.  A referenced set without the key fails as the single-key call does
 * (HIPBFV_E_INVALIDARG before anything is launched; hipbfv_last_error names the set).  rotate_rows_keys decides per set, as
 * SEAL's rotate_internal does for one set: the direct Galois key when that set holds it, the NAF chain of power-of-two keys
 * otherwise (a set with neither lacks the key); when the referenced sets decide differently the two groups run apart.
 * Items need not be grouped by key: the key-switch kernel walks them in key order, so items of one client share that
 * client's key rows in one XCD's L2; with one key set per item the key (16 K (K+1) N bytes) is part of every item's
 * compulsory traffic. */
long hipbfv_batch_relinearize_keys(void *evaluator, const uint64_t *ct3, void *const *relin_key_sets, uint64_t num_key_sets,
                                   const uint32_t *key_index, uint64_t *out2, uint64_t count, void *stream);
long hipbfv_batch_multiply_relin_keys(void *evaluator, const uint64_t *a, const uint64_t *b, void *const *relin_key_sets,
                                      uint64_t num_key_sets, const uint32_t *key_index, uint64_t *out2, uint64_t count,
                                      void *stream);
/* Sums of products with lazy relinearization: out[g] = sum_t a[g][t] * b[g][t] -- an inner product of two ciphertext vectors,
 * the sum of squares of a variance, a row of a ciphertext matrix product -- with ONE key switch per group instead of one per
 * term.  a, b: u64[groups][terms][2][K][N]; b == a (the same pointer) sums squares, and the operand is extended and transformed
 * once.  out3: u64[groups][3][K][N]; out2: u64[groups][2][K][N].
 *  - Bits: out3[g] is, word for word, the sum (hipbfv_batch_add) of hipbfv_batch_multiply over the group's terms, and out2[g] is
 *    hipbfv_batch_relinearize of that sum.  With terms == 1 the calls give exactly the bits of hipbfv_batch_multiply and
 *    hipbfv_batch_multiply_relin.  The _keys form takes one key set per GROUP (key_index: a HOST array of `groups` entries): group
 *    g gives the bits of the single-key call with relin_key_sets[key_index[g]]; only referenced sets are validated and read, as in
 *    hipbfv_batch_relinearize_keys.
 *  - Refusals, all before anything is launched or written: a NULL a, b, output (or key table) is HIPBFV_E_POINTER; terms == 0 is
 *    HIPBFV_E_INVALIDARG; ANY overlap of the output range with [a, a + groups * terms * 2 K N) or the same range of b is
 *    HIPBFV_E_INVALIDARG (the widths differ: there is no in-place form); key_index[g] >= num_key_sets is HIPBFV_E_INVALIDARG; a
 *    missing relinearization key fails as hipbfv_batch_relinearize(_keys) does.  groups == 0 returns HIPBFV_S_OK, nothing launched.
 *  - Launches: where hipbfv_batch_multiply takes the split kernels for groups * terms items, every term is finished inside the
 *    multiply's last kernel and summed in registers: the 3 K rows of a term are never written.  Elsewhere (N < 4096, N = 32768, a
 *    few items) the terms are multiplied into a staging buffer and folded: the same bits.  The evaluator's chunk setting bounds
 *    the scratch: a chunk is a whole number of groups; a group with more terms than a chunk holds is summed in slices
 *    (hipbfv_debug_multiply_sum_plan).  Asynchronous on `stream`.
 *  - Transparent results: the final sums (out3; out2 for the relinearizing forms) are recorded under GROUP numbers
 *    (hipbfv_batch_status).  A transparent single term inside a sum that is not transparent is NOT detected, where the sequence
 *    of single multiplications would have reported it. */
long hipbfv_batch_multiply_sum(void *evaluator, const uint64_t *a, const uint64_t *b, uint64_t *out3, uint64_t groups,
                               uint64_t terms, void *stream);
long hipbfv_batch_multiply_sum_relin(void *evaluator, const uint64_t *a, const uint64_t *b, void *relin_keys, uint64_t *out2,
                                     uint64_t groups, uint64_t terms, void *stream);
long hipbfv_batch_multiply_sum_relin_keys(void *evaluator, const uint64_t *a, const uint64_t *b, void *const *relin_key_sets,
                                          uint64_t num_key_sets, const uint32_t *key_index, uint64_t *out2, uint64_t groups,
                                          uint64_t terms, void *stream);
/* Weighted sums of products: out3[g] = sum_t weights[t] (.) multiply(a[g][t], b[g][t]) -- any signed, integer-weighted quadratic
 * form (4 n0 n2 - n1^2, ad - bc, sum x^2 - 2 sum xy + sum y^2) with one key switch per group.  Everything the three calls above
 * say holds (layouts, b == a, chunks and slices, refusals, group-numbered transparent results); in addition:
 *  - weights is a HOST array of `terms` entries, shared by every group and read before the call returns (the caller may free it
 *    at once).  Any int32_t is a weight, 0 and INT32_MIN included.  NULL is HIPBFV_E_POINTER, refused like every other refusal
 *    before anything is launched or written.
 *  - Bits: w (.) c multiplies every word of residue row i by (w mod q_i), taken canonically in [0, q_i), mod q_i: what |w|
 *    hipbfv_batch_add calls of the product would give, after hipbfv_batch_negate when w < 0.  The weight is applied to the
 *    finished residues of a term inside the multiply's last kernel, just before they are added; out2[g] is
 *    hipbfv_batch_relinearize of the sum.  With every weight 1 the calls run the launches of the unweighted ones.
 *  - Noise: a weight multiplies the noise of its term by |w| (log2 |w| bits of budget); large weights are for exact modular
 *    arithmetic on the words, not for results that must still decrypt.
 *  - A weighted sum whose c1 (and c2) cancel to zero -- all weights 0, or (+1, -1) on equal terms -- is a transparent result. */
long hipbfv_batch_multiply_sum_weighted(void *evaluator, const uint64_t *a, const uint64_t *b, const int32_t *weights,
                                        uint64_t *out3, uint64_t groups, uint64_t terms, void *stream);
long hipbfv_batch_multiply_sum_weighted_relin(void *evaluator, const uint64_t *a, const uint64_t *b, const int32_t *weights,
                                              void *relin_keys, uint64_t *out2, uint64_t groups, uint64_t terms, void *stream);
long hipbfv_batch_multiply_sum_weighted_relin_keys(void *evaluator, const uint64_t *a, const uint64_t *b, const int32_t *weights,
                                                   void *const *relin_key_sets, uint64_t num_key_sets, const uint32_t *key_index,
                                                   uint64_t *out2, uint64_t groups, uint64_t terms, void *stream);
/* Prepared multiplicands: products that share their second operand -- a ciphertext matrix times a ciphertext vector (out[g] =
 * sum_t A[g][t] * x[t], every x[t] used by all groups), one encrypted query scored against many records, one ciphertext times a
 * batch.  hipbfv_Multiplicand_Create copies `count` ciphertexts (ct2: a device array u64[count][2][K][N]) and, where the parameter
 * set has a split multiply (N = 4096 ... 16384), extends and forward-transforms both polynomials of each ONCE; the four calls
 * below then extend and transform `a` alone.  Nothing is replicated in memory and nothing is transformed twice.
 *  - The object: owned by the caller (hipbfv_Multiplicand_Destroy, which waits for the device); asynchronous on `stream` -- ct2
 *    may be overwritten once the work queued on `stream` has passed it.  It records an event behind its last launch, and every call
 *    that uses it makes its own stream wait on that event: the product may run on another stream without a host synchronisation.
 *    hipbfv_Multiplicand_Count gives `count`, hipbfv_Multiplicand_Bytes the device memory it holds (the copy and, with a split
 *    multiply, 2 (K + S) N words per ciphertext of transformed rows, S = the auxiliary base's size).  It may be used by any number
 *    of calls, on any stream, from any evaluator of the context it was made with.
 *  - b_index is a HOST array of `index_len` entries, read before the call returns: item i multiplies a[i] by prepared ciphertext
 *    b_index[i % index_len]; in the sum forms i = g * terms + t.  {0} broadcasts one ciphertext, {0, ..., terms - 1} is the
 *    matrix-vector product, index_len == count an arbitrary mapping.
 *  - Bits: item i of hipbfv_batch_multiply_shared is, word for word, hipbfv_batch_multiply of a[i] with a copy of that ciphertext;
 *    the other three equal hipbfv_batch_multiply_relin, hipbfv_batch_multiply_sum and hipbfv_batch_multiply_sum_relin on the
 *    replicated array.  The path (split kernels or whole-polynomial kernels, fused relinearization, chunks and slices) is the
 *    counterpart's for the same item count; off the split path the chunk's multiplicands are gathered from the object's copy.
 *  - Refusals, all before anything is launched or written: a NULL a, output, multiplicand or b_index is HIPBFV_E_POINTER;
 *    index_len == 0, terms == 0 or an index >= the object's count is HIPBFV_E_INVALIDARG (hipbfv_last_error names the first such
 *    item); so is a multiplicand made by an evaluator of another context; a missing relinearization key fails as in the
 *    counterpart.  Aliasing: out2 of hipbfv_batch_multiply_relin_shared may be exactly `a`; any other overlap of an output with `a`
 *    is HIPBFV_E_INVALIDARG.  count == 0 / groups == 0 returns HIPBFV_S_OK with no launch; hipbfv_Multiplicand_Create with
 *    count == 0 is HIPBFV_E_INVALIDARG.
 *  - Transparent results are recorded as in the counterparts: by item number, by GROUP number in the sum forms. */
long hipbfv_Multiplicand_Create(void *evaluator, const uint64_t *ct2, uint64_t count, void *stream, void **multiplicand);
long hipbfv_Multiplicand_Destroy(void *multiplicand);
long hipbfv_Multiplicand_Count(void *multiplicand, uint64_t *count);
long hipbfv_Multiplicand_Bytes(void *multiplicand, uint64_t *bytes);
long hipbfv_batch_multiply_shared(void *evaluator, const uint64_t *a, void *multiplicand, const uint32_t *b_index, uint64_t index_len,
                                  uint64_t *out3, uint64_t count, void *stream);
long hipbfv_batch_multiply_relin_shared(void *evaluator, const uint64_t *a, void *multiplicand, const uint32_t *b_index, uint64_t index_len,
                                        void *relin_keys, uint64_t *out2, uint64_t count, void *stream);
long hipbfv_batch_multiply_sum_shared(void *evaluator, const uint64_t *a, void *multiplicand, const uint32_t *b_index, uint64_t index_len,
                                      uint64_t *out3, uint64_t groups, uint64_t terms, void *stream);
long hipbfv_batch_multiply_sum_relin_shared(void *evaluator, const uint64_t *a, void *multiplicand, const uint32_t *b_index,
                                            uint64_t index_len, void *relin_keys, uint64_t *out2, uint64_t groups, uint64_t terms, void *stream);
/* Products of TWO prepared operands: both operands recur -- the ciphertext matrix product C = A B (C[i][j] = sum_t A[i][t] * B[t][j]:
 * every A[i][t] is used by n groups, every B[t][j] by m), a Gram matrix, all-pairs scoring of two ciphertext sets.  ma and mb are
 * ordinary multiplicand objects (hipbfv_Multiplicand_Create; ma == mb is allowed): each distinct ciphertext was extended and
 * forward-transformed once when its object was made, and these calls extend and transform nothing.
 *  - a_index and b_index are HOST arrays of `index_len` entries each, read before the call returns: item i multiplies prepared
 *    ciphertext a_index[i % index_len] of ma by prepared ciphertext b_index[i % index_len] of mb; in the sum forms i = g * terms + t.
 *  - Bits: every output is, word for word, the counterpart call (hipbfv_batch_multiply, hipbfv_batch_multiply_relin,
 *    hipbfv_batch_multiply_sum, hipbfv_batch_multiply_sum_relin) on the two gathered arrays; an item whose two operands are the same
 *    prepared ciphertext has the words of the product of that ciphertext with itself.
 *  - Path: the counterpart's for the same item count.  Where that is the split kernels (and both objects hold transformed rows)
 *    there is no head launch at all: one middle kernel reads both operands' rows, forms the three products and runs the inverse
 *    transforms; the tail, the summing tail and the fused relinearization are the counterpart's.  Elsewhere (N < 4096, N = 32768, a
 *    few items) both operands of a chunk are gathered from the objects' copies and the counterpart's launches run.
 *  - Refusals, all before anything is launched, copied or written: a NULL evaluator, ma, mb, a_index, b_index or output, or a handle
 *    that is not a multiplicand, is HIPBFV_E_POINTER; index_len == 0, terms == 0 or an index >= its object's count is
 *    HIPBFV_E_INVALIDARG (hipbfv_last_error names the first such item as "item <i>" and the operand as a_index or b_index); so is an
 *    object made for another context; a missing relinearization key fails as in the counterpart.  The objects own the operands, so
 *    an output cannot alias them.  count == 0 / groups == 0 returns HIPBFV_S_OK with no launch.
 *  - Transparent results are recorded as in the counterparts: by item number, by GROUP number in the sum forms. */
long hipbfv_batch_multiply_prepared(void *evaluator, void *ma, const uint32_t *a_index, void *mb, const uint32_t *b_index, uint64_t index_len,
                                    uint64_t *out3, uint64_t count, void *stream);
long hipbfv_batch_multiply_relin_prepared(void *evaluator, void *ma, const uint32_t *a_index, void *mb, const uint32_t *b_index,
                                          uint64_t index_len, void *relin_keys, uint64_t *out2, uint64_t count, void *stream);
long hipbfv_batch_multiply_sum_prepared(void *evaluator, void *ma, const uint32_t *a_index, void *mb, const uint32_t *b_index,
                                        uint64_t index_len, uint64_t *out3, uint64_t groups, uint64_t terms, void *stream);
long hipbfv_batch_multiply_sum_relin_prepared(void *evaluator, void *ma, const uint32_t *a_index, void *mb, const uint32_t *b_index,
                                              uint64_t index_len, void *relin_keys, uint64_t *out2, uint64_t groups, uint64_t terms,
                                              void *stream);
long hipbfv_batch_apply_galois_keys(void *evaluator, const uint64_t *ct2, uint32_t galois_elt, void *const *galois_key_sets,
                                    uint64_t num_key_sets, const uint32_t *key_index, uint64_t *out2, uint64_t count,
                                    void *stream);
long hipbfv_batch_rotate_rows_keys(void *evaluator, const uint64_t *ct2, int steps, void *const *galois_key_sets,
                                   uint64_t num_key_sets, const uint32_t *key_index, uint64_t *out2, uint64_t count,
                                   void *stream);
long hipbfv_batch_rotate_columns_keys(void *evaluator, const uint64_t *ct2, void *const *galois_key_sets,
                                      uint64_t num_key_sets, const uint32_t *key_index, uint64_t *out2, uint64_t count,
                                      void *stream);
/* Mixed-step rotation batches with one key set per client: the two families above at once.  Item i is rotated by its own
 * steps[i] (galois_elts[i]) through key set key_index[i] -- the ready queue of a multi-tenant server, as it stands, in ONE call.
 * steps / galois_elts / key_index and the handle array are HOST arrays, read before the call returns.
 *  - Bits: item i has exactly the words of hipbfv_batch_rotate_rows(..., steps[i], key_sets[key_index[i]], ...) called on that
 *    item alone (apply_galois_items_keys: of hipbfv_batch_apply_galois with galois_elts[i]), whoever else is in the batch and
 *    whatever the order of the items.
 *  - Decisions stay per (set, step): step 0 / element 1 copies the item; a set that holds the step's direct key rotates through
 *    it; a set without it takes the NAF chain of power-of-two keys (SEAL's rotate_internal; the part of n/2 rows is skipped).
 *    Two clients with the same step may decide differently within one call.
 *  - Launches: ALL items that rotate through a direct key -- every client, every step -- share one key-switch launch sequence
 *    per chunk; its key table has one entry per (element, set) pair and is walked in that order.  All chain items of the call
 *    are gathered once and share their rounds: round r rotates every unfinished item by the r-th part of its own chain through
 *    its own client's key in one launch sequence, so the call runs as many rounds as its longest chain has parts
 *    (hipbfv_debug_rotate_items_keys_plan).
 *  - Only referenced sets count.  A set is referenced only by an item that needs a key: items that copy reference nothing, and
 *    their set may be NULL or foreign.  key_index[i] >= num_key_sets is refused for every item, copied ones included.
 *  - Refusals are HIPBFV_E_INVALIDARG: |step| >= N/2; an even or too large element; a referenced set that is NULL, not a key
 *    object, of another context, or that lacks the direct key and also a key of the chain.  Every refusal comes before anything
 *    is launched, copied or written, and hipbfv_last_error reads "item <i>: key set <k>: ..." for the first offending item, k in
 *    the caller's numbering.
 *  - Aliasing as above: out2 may be exactly ct2, any other overlap is refused.  Parameters without batching give
 *    COR_E_INVALIDOPERATION for the row rotations; count == 0 returns S_OK.  Transparent results are recorded as in the sibling
 *    calls (hipbfv_batch_status), under the caller's item numbers. */
long hipbfv_batch_apply_galois_items_keys(void *evaluator, const uint64_t *ct2, const uint32_t *galois_elts,
                                          void *const *galois_key_sets, uint64_t num_key_sets, const uint32_t *key_index,
                                          uint64_t *out2, uint64_t count, void *stream);
long hipbfv_batch_rotate_rows_items_keys(void *evaluator, const uint64_t *ct2, const int32_t *steps,
                                         void *const *galois_key_sets, uint64_t num_key_sets, const uint32_t *key_index,
                                         uint64_t *out2, uint64_t count, void *stream);
long hipbfv_batch_add(void *evaluator, const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t size,
                      uint64_t count, void *stream);
long hipbfv_batch_sub(void *evaluator, const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t size,
                      uint64_t count, void *stream);
long hipbfv_batch_negate(void *evaluator, const uint64_t *a, uint64_t *out, uint64_t size, uint64_t count, void *stream);
/* plain: device u64[count][N] (plain_stride = N) or one shared plaintext (plain_stride = 0) */
long hipbfv_batch_add_plain(void *evaluator, const uint64_t *ct, uint64_t size, const uint64_t *plain,
                            uint64_t plain_stride, uint64_t *out, uint64_t count, void *stream);
long hipbfv_batch_sub_plain(void *evaluator, const uint64_t *ct, uint64_t size, const uint64_t *plain,
                            uint64_t plain_stride, uint64_t *out, uint64_t count, void *stream);
long hipbfv_batch_multiply_plain(void *evaluator, const uint64_t *ct, uint64_t size, const uint64_t *plain,
                                 uint64_t plain_stride, uint64_t *out, uint64_t count, void *stream);
/* forward / inverse negacyclic NTT of u64[polys][N]; polynomial p uses key-level prime (p % nprimes) */
long hipbfv_batch_ntt(void *evaluator, uint64_t *data, uint64_t polys, uint64_t nprimes, bool inverse, void *stream);
/* ct u64[count][size][K][N] -> out u64[count][size][K-1][N] (the layout of hipbfv_Context_NextLevel's context) */
long hipbfv_batch_mod_switch(void *evaluator, const uint64_t *ct, uint64_t size, uint64_t *out, uint64_t count, void *stream);
/* The steps either side of the evaluator, batched on device buffers:
 * encode / decode: values u64[count][N] (int64 when is_signed) <-> plaintexts u64[count][N];
 * decrypt: ct u64[count][size][K][N] -> plaintexts u64[count][N] (zero padded);
 * encrypt: plaintexts u64[count][N] (plain_stride = N) or one shared (0) -> ct u64[count][2][K][N]; item i draws its
 * randomness from the ChaCha20 blocks at position first_op + i under the seed (distinct (seed, op) pairs give independent
 * randomness; the generator is described in sunscreen_amd/csrc/rng.hpp).  hipbfv_batch_encrypt_seeded takes the 512-bit
 * seed SEAL's prng_seed_type carries (64 bytes; NULL = 512 fresh bits from getrandom(2), failing with E_UNEXPECTED if
 * the OS has none) and is the production entry point.  hipbfv_batch_encrypt with its 64-bit `seed` is TEST ONLY
 * (reproducible batches for the parity tests: 2^64 candidates can be searched), like hipbfv_Encryptor_SetSeed,
 * hipbfv_KeyGenerator_SetSeed and hipbfv_KeyGenerator_CreateSeeded.
 * encode synchronises the stream (it reports out-of-range values); the others are asynchronous. */
long hipbfv_batch_encode(void *evaluator, const uint64_t *values, uint64_t *plain, uint64_t count, int is_signed, void *stream);
long hipbfv_batch_decode(void *evaluator, const uint64_t *plain, uint64_t *values, uint64_t count, int is_signed, void *stream);
long hipbfv_batch_decrypt(void *evaluator, const uint64_t *ct, uint32_t size, void *secret_key, uint64_t *plain, uint64_t count, void *stream);
/* Invariant noise on device batches (Decryptor_InvariantNoiseBudget / Decryptor_InvariantNoise per item, from the phase that
 * decrypt computes): budget int32_t[count] = max(0, bits(q) - bits(max_x |[t * ct(s)(x)]_q|) - 1), the centred norm taken exactly;
 * noise double[count] (nullable) = that norm / q.  decrypt_checked writes the plaintexts of hipbfv_batch_decrypt (the same bits)
 * and the budgets of noise_budget from ONE phase computation: an item with budget 0 decrypted to garbage (the reference's
 * Runtime::decrypt returns Error::TooMuchNoise for it).  hipbfv_batch_decrypt's key and level rules; NULL required pointer:
 * HIPBFV_E_POINTER; size < 2: HIPBFV_E_INVALIDARG; count == 0: HIPBFV_S_OK, nothing launched.  Asynchronous on `stream`; the
 * evaluator's status word is not touched (budget is the only report). */
long hipbfv_batch_noise_budget(void *evaluator, const uint64_t *ct, uint32_t size, void *secret_key, int32_t *budget, double *noise,
                               uint64_t count, void *stream);
long hipbfv_batch_decrypt_checked(void *evaluator, const uint64_t *ct, uint32_t size, void *secret_key, uint64_t *plain, int32_t *budget,
                                  uint64_t count, void *stream);
long hipbfv_batch_encrypt(void *evaluator, const uint64_t *plain, uint64_t plain_stride, void *public_key, uint64_t seed, uint64_t first_op,
                          uint64_t *ct, uint64_t count, void *stream);
long hipbfv_batch_encrypt_seeded(void *evaluator, const uint64_t *plain, uint64_t plain_stride, void *public_key, const uint8_t *seed64,
                                 uint64_t first_op, uint64_t *ct, uint64_t count, void *stream);
/* Plaintext-matrix x ciphertext-vector products in the transform domain -- the first loop nest of examples/pir
 * (examples/pir/src/main.rs:16-45: col[i] = sum_j database[i][j] * col_query[j]).  plain_to_ntt transforms plaintexts
 * the way Evaluator_MultiplyPlain does internally (a static database is transformed once); ct_to_ntt transforms every
 * polynomial of the ciphertexts; dot_plain_ntt produces, for size-2 ciphertexts, out[row] = sum_j MultiplyPlain(ct_j,
 * plain[row][j]) in coefficient form, bit-identical to the reference's sequence of multiply_plain and add.
 * ctn: u64[cols][2][K][N], pntt: u64[rows][cols][K][N], out: u64[rows][2][K][N].
 * An ALL-ZERO plaintext has no transformed form: SEAL refuses every product with it (transparent result), and the consumers
 * of `pntt` cannot see it any more, so plain_to_ntt records the index of the first all-zero plaintext in the evaluator's
 * status word -- hipbfv_batch_status returns COR_E_INVALIDOPERATION for it, as for any transparent batch result. */
long hipbfv_batch_plain_to_ntt(void *evaluator, const uint64_t *plain, uint64_t plain_stride, uint64_t *pntt, uint64_t count, void *stream);
long hipbfv_batch_ct_to_ntt(void *evaluator, const uint64_t *ct, uint64_t size, uint64_t *ctn, uint64_t count, void *stream);
long hipbfv_batch_dot_plain_ntt(void *evaluator, const uint64_t *ctn, uint64_t cols, const uint64_t *pntt, uint64_t rows, uint64_t *out,
                                void *stream);
/* Many queries against ONE pass over the database: every database word is loaded once and multiplied against a tile of queries.
 * out[q] is, word for word, hipbfv_batch_dot_plain_ntt(ctn + q * cols * 2 * K * N, cols, pntt, rows) -- the reference's sequence of
 * multiply_plain and add for query q (every step is exact modular arithmetic: tile shape and summation order cannot show).  out
 * is laid out as hipbfv_batch_multiply_sum_relin_keys takes a[groups = queries][terms = rows].
 * ctn: u64[queries][cols][2][K][N] (ct_to_ntt), pntt: u64[rows][cols][K][N] (plain_to_ntt),
 * out: u64[queries][rows][2][K][N], coefficient form.
 * A NULL pointer is HIPBFV_E_POINTER; cols == 0, rows == 0, an argument beyond 2^32 - 1 or any overlap of the output range with
 * the ctn or pntt range is HIPBFV_E_INVALIDARG; queries == 0 is HIPBFV_S_OK.  Nothing is launched or written in any of these
 * cases.  Asynchronous on `stream`. */
long hipbfv_batch_dot_plain_ntt_queries(void *evaluator, const uint64_t *ctn, uint64_t queries, uint64_t cols, const uint64_t *pntt,
                                        uint64_t rows, uint64_t *out, void *stream);
long hipbfv_set_chunk_ops(void *evaluator, uint64_t chunk_ops);

/* Batch executor for compiled FHE program graphs (replaces sunscreen_runtime/src/run.rs:100-357).
 * Node kinds follow sunscreen_fhe_program::Operation (operation.rs:12-94) in this order:
 * 0 ShiftLeft, 1 ShiftRight, 2 SwapRows, 3 Relinearize, 4 Multiply, 5 MultiplyPlaintext, 6 Add,
 * 7 AddPlaintext, 8 Negate, 9 Sub, 10 SubPlaintext, 11 InputCiphertext(arg), 12 InputPlaintext(arg),
 * 13 Literal::U64(arg), 14 OutputCiphertext (15 Literal::Plaintext: hipbfv_Program_AddPlaintextLiteral / JSON only).
 * Edge kinds: 0 Left, 1 Right, 2 Unary.
 * LoadJson accepts the serde JSON form of `FheProgram` (petgraph StableGraph).
 * Run executes the graph over `batch` independent input sets: input i is a device pointer to
 * u64[batch][2][K][N] (kind 0), to plaintexts u64[batch][N] / one shared u64[N] (kind 1, stride N / 0), or to plaintexts
 * already lifted and transformed, u64[batch][K][N] / one shared u64[K][N] (kind 2, stride K*N / 0: the output of
 * hipbfv_batch_plain_to_ntt -- static data such as examples/pir's database is transformed once, not per query; only
 * MultiplyPlaintext nodes may consume it, and its zero check is the producer's: hipbfv_batch_plain_to_ntt + hipbfv_batch_status);
 * one output buffer u64[batch][2][K][N] per OutputCiphertext node, in node order.
 * Execution follows the reference's `traverse` (sunscreen_runtime/src/run.rs:372-472: every node whose operands are
 * complete runs at once): ready nodes of one kind are one batched launch, Add / Sub / Negate trees are n-ary sums, sums of
 * ciphertext-plaintext products stay in the transform domain (program_plan.cpp).  Bits are those of the node-by-node
 * evaluation; HIPBFV_PROGRAM_SERIAL=1 selects that executor (one node at a time, kinds 0 / 1 only).
 *
 * Transparent results (SEAL built with SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT, seal_fhe/build.rs:46-66: `runtime.run` fails
 * on `a * 0`, sunscreen/tests/features.rs:8-34).  The handle-level Evaluator_* functions check their one result before
 * they return.  The batched paths check on the device: every operation records, in a status word, the smallest batch
 * index whose result is transparent.  Program_Run owns such a word per run, reads it once at exit (one stream
 * synchronisation per run) and returns COR_E_INVALIDOPERATION -- hipbfv_last_error names AN input set whose result is
 * transparent (merged launches number their ciphertexts member-major, so it need not be the lowest such set).  The
 * hipbfv_batch_* operations stay asynchronous on `stream` and record into their evaluator's word; hipbfv_batch_status
 * synchronises `stream`, reads and resets it: COR_E_INVALIDOPERATION + the first transparent item (of any operation since
 * the previous call), S_OK + ~0 otherwise.  hipbfv_set_batch_transparent_check(evaluator, false) switches the recording
 * off for one evaluator; hipbfv_set_throw_on_transparent(false) for the whole library (the crate's
 * `transparent-ciphertexts` feature). */
long hipbfv_Program_Create(void **program);
long hipbfv_Program_Destroy(void *program);
long hipbfv_Program_AddNode(void *program, uint32_t op, uint64_t arg, uint32_t *node_id);
/* Literal::Plaintext(bytes) node: `bytes` is what the compiler stores in the graph -- bincode of
 * InnerPlaintext::Seal([WithContext{Params, SEAL-serialised Plaintext}]) (sunscreen_fhe_program/src/literal.rs:8-18,
 * sunscreen/src/fhe/mod.rs:370-376, decoded by the reference at sunscreen_runtime/src/run.rs:312-328).  The
 * parameters inside are checked against the evaluator's context when the program runs. */
long hipbfv_Program_AddPlaintextLiteral(void *program, const uint8_t *bytes, uint64_t length, uint32_t *node_id);
long hipbfv_Program_AddEdge(void *program, uint32_t src, uint32_t dst, uint32_t kind);
long hipbfv_Program_LoadJson(void *program, const char *json, uint64_t length);
long hipbfv_batch_status(void *evaluator, uint64_t *first_transparent_item, void *stream);
long hipbfv_set_batch_transparent_check(void *evaluator, bool enabled);
long hipbfv_Program_NumOutputs(void *program, uint64_t *count);
/* Diagnostic: one multiply + relinearize of ONE ciphertext pair (device pointers u64[2][K][N], a relinearisation key
 * u64[K][2][K+1][N], result u64[2][K][N]) timed from the host, launched kernel by kernel and replayed from a captured hipGraph
 * (microseconds per repetition, one stream synchronisation each). */
long hipbfv_debug_graph_probe(void *context, const uint64_t *a, const uint64_t *b, const uint64_t *relin_key, uint64_t *out,
                              uint64_t iterations, double *us_direct, double *us_graph);
/* Diagnostic, host only (no device): the FP64 range plans of one prime at degree 2^log_n -- out6 = {FP64 policy possible,
 * forward reduce mask, inverse reduce mask, split pipelines possible, split forward mask, split inverse mask}; bit p of a mask =
 * every value is reduced mod q at the start of pass p (bit 8 of the split inverse mask: at the start of the tail stages). */
long hipbfv_debug_f64_plan(uint64_t prime, uint32_t log_n, uint32_t *out6);
/* Diagnostic, host only (no device): the auxiliary base a context with these parameters gets -- the same values
 * hipbfv_Context_AuxBase reports for a live context (B, then m_sk last), `flags` likewise.  tests/test_behz_base_bound_cpu.py
 * replays the BEHZ floor and Shenoy-Kumaresan steps in exact integers over the base returned here. */
long hipbfv_debug_aux_base(uint64_t poly_modulus_degree, const uint64_t *coeff_primes, uint64_t prime_count, uint64_t plain_modulus,
                           uint64_t *count, uint64_t *primes, uint64_t capacity, int *flags);
/* The schedule Run follows, one line per step ("mul_relin members=3 square", "sum members=2 terms=6", "plain_matrix members=256
 * columns=256", ...): `*needed` = bytes including the terminator; `buffer` may be NULL to ask for the size. */
long hipbfv_Program_Describe(void *program, char *buffer, uint64_t capacity, uint64_t *needed);
/* Run: one stream synchronisation per 32768 input sets (the status word is read once per such chunk; batches up to 32768 --
 * every BASELINE configuration -- synchronise once, at exit).  A batch above 32768 runs as consecutive chunks over offset
 * pointers: a failure or a transparent result in chunk k returns its error with the outputs of chunks 0 .. k-1 already written. */
long hipbfv_Program_Run(void *program, void *evaluator, uint64_t batch, uint64_t num_inputs, const uint32_t *input_kinds,
                        const uint64_t *const *input_ptrs, const uint64_t *input_strides, void *relin_keys,
                        void *galois_keys, uint64_t num_outputs, uint64_t *const *outputs, void *stream);

/* Run with one key set per client: input set i of the batch uses relin_keys[key_index[i]] / galois_keys[key_index[i]]
 * (HOST arrays: num_key_sets handles each -- an entry may be NULL when the program needs no such key -- and `batch`
 * indices).  Same bits per input set as hipbfv_Program_Run with that set's keys alone (the reference's call,
 * run.rs:100-105), whoever else is in the batch.  Only the referenced sets count, as in the per-key batches above: an
 * unreferenced entry may be anything, a referenced handle that is not a key object of the evaluator's context is
 * HIPBFV_E_INVALIDARG (naming the set).  Input sets whose key sets hold different kinds of keys (a relinearisation key or
 * not, which Galois elements) run as separate runs, one per kind, gathered and scattered through scratch buffers. */
long hipbfv_Program_RunKeys(void *program, void *evaluator, uint64_t batch, uint64_t num_inputs, const uint32_t *input_kinds,
                            const uint64_t *const *input_ptrs, const uint64_t *input_strides, uint64_t num_key_sets,
                            void *const *relin_keys, void *const *galois_keys, const uint32_t *key_index,
                            uint64_t num_outputs, uint64_t *const *outputs, void *stream);

/* Device pool: HOST-fed batches sharded over several devices (sunscreen_amd/csrc/pool.hpp).
 * Members run on devices[0..count); an ordinal may repeat (several members on one device).  Every member has its own
 * context, built from `context`'s parameters (the same auxiliary base and HIPBFV_SEAL_AUX rule, so the same bits), its own
 * evaluator, three streams (in / compute / out), device buffers for three chunks in flight, pinned bounce buffers and one
 * worker thread.  Members are not contexts of the process: they do not count for hipbfv_set_device, and they never use the
 * process's cached device blocks.
 *  - Synchronous: a call returns when every output is in host memory.  Calls on one pool are serialised; calls on
 *    different pools run concurrently.
 *  - Sharding: contiguous blocks whose sizes differ by at most one (sunscreen_amd/dist.py:shard_range), one per member; an
 *    empty shard launches nothing; batch 0 is S_OK.
 *  - Bits: input set i gives exactly the bits of hipbfv_batch_multiply_relin / hipbfv_Program_Run on input set i, whatever
 *    the member count, the chunk size, or whether the host memory is pinned.
 *  - Keys: the existing key handles, of any context with the pool's parameters.  A member copies a key's device data on the
 *    first call that needs it there (peer copy across devices, device-to-device on the same device) and keeps the copy while
 *    the key buffer lives.  A key of other parameters counts as absent; a missing key fails before anything is launched.
 *  - Host memory: buffers hipPointerGetAttributes reports as pinned are copied from directly; other host memory is staged
 *    through the member's pinned bounce buffers; device pointers are E_INVALIDARG.
 *  - A transparent result is COR_E_INVALIDOPERATION (while hipbfv_set_throw_on_transparent is on), and hipbfv_last_error
 *    names the input set's index in the whole batch.  A failure leaves the pool usable. */
long hipbfv_Pool_Create(void *context, const int *devices, uint32_t count, void **pool);
long hipbfv_Pool_Destroy(void *pool);
/* input sets per pipeline chunk per member; 0 = the library's choice (default: 2^21 / N, 256 at N = 8192) */
long hipbfv_Pool_SetChunk(void *pool, uint64_t sets_per_chunk);
/* one line per member: "member=0 device=0 chunk=256 key_copies=1 keys_cached=1 slot_words=... bounce_words=... key_bytes=...
 * key_evictions=..."
 * (*needed = length + 1 as in hipbfv_Program_Describe; buffer may be NULL) */
long hipbfv_Pool_Describe(void *pool, char *buffer, uint64_t capacity, uint64_t *needed);
/* HOST pointers, u64[count][2][K][N]; out = relinearize(a * b); the aliasing rule of hipbfv_batch_multiply_relin */
long hipbfv_Pool_MultiplyRelin(void *pool, const uint64_t *a, const uint64_t *b, void *relin_keys, uint64_t *out, uint64_t count);
/* hipbfv_Program_Run over HOST inputs and outputs: kinds 0 and 1 (stride 0 = one shared plaintext, copied to each member
 * once per call); kind 2 is E_INVALIDARG */
long hipbfv_Pool_ProgramRun(void *pool, void *program, uint64_t batch, uint64_t num_inputs, const uint32_t *input_kinds,
                            const uint64_t *const *input_ptrs, const uint64_t *input_strides, void *relin_keys,
                            void *galois_keys, uint64_t num_outputs, uint64_t *const *outputs);
/* Per-client key sets through the pool: input set i uses key set key_index[i], as in hipbfv_batch_*_keys and
 * hipbfv_Program_RunKeys, whose argument order these follow (no evaluator, no stream; HOST data pointers; the handle arrays
 * and key_index are host arrays as there).  One shared key set is num_key_sets = 1 with an all-zero key_index.
 *  - Bits: input set i gives exactly the words of hipbfv_batch_multiply_relin_keys / hipbfv_batch_rotate_rows_keys /
 *    hipbfv_batch_rotate_columns_keys / hipbfv_Program_RunKeys over the whole batch on one device -- hence of the single-key
 *    call with key_sets[key_index[i]] -- whatever the member count, the chunk size, the order of clients in the batch, whether
 *    the host memory is pinned, and whatever the key-cache bound.
 *  - Sharding: as above; key_index is sliced with the input sets, which need not be grouped by client.
 *  - Only referenced sets count: an entry no key_index entry names may be NULL, foreign or lack the key.  A referenced set that
 *    is NULL, not a key object, of other parameters, or without a key the call needs (the relinearisation key; the direct
 *    Galois key of `steps` or else every power-of-two key of its NAF chain; what the program's graph needs) is
 *    HIPBFV_E_INVALIDARG and hipbfv_last_error names the set's index in the CALLER's array; key_index[i] >= num_key_sets
 *    likewise.  This is decided on the calling thread over the whole batch before any member copies or launches anything:
 *    outputs are untouched and no key is copied.
 *  - Per-set decisions stay per set: in RotateRowsKeys a set that holds the direct key uses it and a set without takes the NAF
 *    chain, both in one call; in ProgramRunKeys input sets whose key sets hold different kinds of keys run as separate runs
 *    inside the member, as in hipbfv_Program_RunKeys.
 *  - What a member copies: for every pipeline chunk, the distinct sets the chunk's key_index names become the chunk's own
 *    handle table and key_index is remapped onto it (hipbfv_debug_pool_keyplan).  A member copies a key buffer only if a set
 *    of its own shard references it AND the call needs that key: index 0 for MultiplyRelinKeys; the Galois elements the
 *    rotation reads for that set; for a program the relinearisation key if the graph relinearises and the set's Galois
 *    elements if it rotates.  Copies are made once and kept while the key buffer lives (or until the bound drops them).
 *  - hipbfv_Pool_SetKeyCacheBytes: a bound, per member, on the bytes of key copies it keeps; 0 = no bound (the default).  It
 *    holds from the next call on, for every pool call.  Before a chunk's keys are staged the member drops least-recently-used
 *    copies that no chunk in flight references until the chunk's keys fit; a chunk whose own keys exceed the bound is
 *    HIPBFV_E_OUTOFMEMORY, the message giving both byte counts (lower hipbfv_Pool_SetChunk or raise the bound).
 *    hipbfv_Pool_Describe ends every member line with "key_bytes=... key_evictions=...".
 *  - Transparent results, failures, serialisation, kind-2 inputs and device pointers: as for the calls above.
 *  - Aliasing: out == a (out2 == ct2) exactly is allowed as in the batched calls; any other overlap of the host ranges is
 *    HIPBFV_E_INVALIDARG before anything runs. */
long hipbfv_Pool_MultiplyRelinKeys(void *pool, const uint64_t *a, const uint64_t *b, void *const *relin_key_sets,
                                   uint64_t num_key_sets, const uint32_t *key_index, uint64_t *out, uint64_t count);
long hipbfv_Pool_RotateRowsKeys(void *pool, const uint64_t *ct2, int steps, void *const *galois_key_sets, uint64_t num_key_sets,
                                const uint32_t *key_index, uint64_t *out2, uint64_t count);
long hipbfv_Pool_RotateColumnsKeys(void *pool, const uint64_t *ct2, void *const *galois_key_sets, uint64_t num_key_sets,
                                   const uint32_t *key_index, uint64_t *out2, uint64_t count);
long hipbfv_Pool_ProgramRunKeys(void *pool, void *program, uint64_t batch, uint64_t num_inputs, const uint32_t *input_kinds,
                                const uint64_t *const *input_ptrs, const uint64_t *input_strides, uint64_t num_key_sets,
                                void *const *relin_keys, void *const *galois_keys, const uint32_t *key_index,
                                uint64_t num_outputs, uint64_t *const *outputs);
long hipbfv_Pool_SetKeyCacheBytes(void *pool, uint64_t bytes);
/* hipbfv_batch_rotate_rows_items_keys through the pool: input set i by steps[i] with key set key_index[i] (HOST data pointers and
 * host arrays, no evaluator, no stream).  Input set i has exactly the words of the one-device call -- hence of
 * hipbfv_batch_rotate_rows on that set alone with its client's keys -- whatever the member count, the chunk size, the order of the
 * clients, the kind of host memory and the key-cache bound.  steps and key_index are sliced with the input sets.  Every refusal
 * of the one-device call (same text: "item <i>: key set <k>: ...", i the index in the whole batch, k in the caller's array; "of
 * another context" reads "other encryption parameters" here) is decided on the calling thread over the whole batch before any
 * member copies a key or launches anything.  A member copies, per chunk, only the Galois keys the chunk's own (set, step) pairs
 * read: the direct key, or the chain's.  The key-cache bound, eviction, transparent results (the message names the batch-wide
 * index), aliasing, failures and serialisation are those of the calls above. */
long hipbfv_Pool_RotateRowsItemsKeys(void *pool, const uint64_t *ct2, const int32_t *steps, void *const *galois_key_sets,
                                     uint64_t num_key_sets, const uint32_t *key_index, uint64_t *out2, uint64_t count);
/* the pool's shard rule, host only: member `member` of `members` gets input sets [*begin, *end) of a batch */
long hipbfv_debug_pool_shard(uint64_t batch, uint32_t members, uint32_t member, uint64_t *begin, uint64_t *end);
/* the pool's per-chunk key table, host only: for chunk `chunk_no` of member `member`'s shard (`chunk` input sets per chunk, at
 * most the shard), local_sets[0, *local_count) = the distinct key sets the chunk names, ascending in the caller's numbering
 * (capacity num_key_sets), and remapped[0, *sets_in_chunk) = the chunk's key_index as indices into local_sets (capacity
 * `chunk`).  A member, a chunk number or a key index out of range is HIPBFV_E_INVALIDARG. */
long hipbfv_debug_pool_keyplan(const uint32_t *key_index, uint64_t batch, uint64_t num_key_sets, uint32_t members, uint32_t member,
                               uint64_t chunk, uint64_t chunk_no, uint32_t *local_sets, uint64_t *local_count,
                               uint32_t *remapped, uint64_t *sets_in_chunk);
/* Host only: what hipbfv_batch_rotate_rows_items does with `steps` at degree n over a key set that holds exactly the keys of the
 * elements present_elts -- kind[i]: 0 the item is copied, 1 it goes into the mixed launch (group[i] = its Galois element), 2 it
 * joins NAF chain group group[i] (groups numbered in the order their step first appears; *chain_groups of them).  Fails as the
 * call would (a refused step, a missing key; the message names the item). */
long hipbfv_debug_rotate_items_plan(uint64_t n, const int32_t *steps, uint64_t count, const uint32_t *present_elts,
                                    uint64_t num_present, int32_t *kind, uint32_t *group, uint64_t *chain_groups);
/* Host only: what hipbfv_batch_rotate_rows_items_keys does with (steps, key_index) at degree n where key set k holds exactly the
 * keys of the elements present_elts[present_offsets[k], present_offsets[k + 1]) (num_key_sets + 1 offsets).  kind[i]: 0 the item
 * is copied, 1 it goes into the mixed launch through entry table_entry[i] of its key table (*table_entries entries, numbered by
 * (element, set)), 2 it runs a NAF chain of chain_rounds_of_item[i] rounds (0 for the other kinds).  *rounds: the rounds the call
 * runs, the longest chain's.  Fails as the call would; the message names the item and the set. */
long hipbfv_debug_rotate_items_keys_plan(uint64_t n, const int32_t *steps, const uint32_t *key_index, uint64_t count,
                                         uint64_t num_key_sets, const uint32_t *present_elts, const uint64_t *present_offsets,
                                         int32_t *kind, uint32_t *table_entry, uint32_t *chain_rounds_of_item,
                                         uint64_t *table_entries, uint64_t *rounds);
/* Host only: the launch sequences of hipbfv_batch_multiply_sum(_relin) for `groups` groups of `terms` terms under a chunk of
 * `chunk` items (at most 65535 count).  steps5[i] = {first group, groups, first term, terms, accumulate} of sequence i (capacity
 * rows of five): its items are multiplied together and summed by one launch; accumulate = 1: the sums are added onto the rows an
 * earlier slice of the same group wrote.  *count = the number of sequences (E_INVALIDARG when it exceeds capacity). */
long hipbfv_debug_multiply_sum_plan(uint64_t groups, uint64_t terms, uint64_t chunk, uint64_t *steps5, uint64_t capacity,
                                    uint64_t *count);
/* Host only: what hipbfv_batch_rotate_rows_sum does with `steps` (terms entries) at degree n over a key set that holds exactly the
 * keys of the elements present_elts, for `groups` groups under a chunk of `chunk` items.  kind[t]: 0 the term is the source itself,
 * 1 it rotates through its own key inside the summing sequence (elt[t] = its Galois element), 2 it walks a NAF chain of rounds[t]
 * hops beforehand and enters the sum as an identity term (rounds[t] = 0 for the other kinds).  steps5 / capacity / *count: the launch
 * sequences as rows of {first group, groups, first term, terms, accumulate}, exactly as hipbfv_debug_multiply_sum_plan reports them.
 * Fails as the call would (terms == 0, a refused step or a missing key: "term <t>: ..."), and on chunk == 0. */
long hipbfv_debug_rotate_sum_plan(uint64_t n, const int32_t *steps, uint64_t terms, const uint32_t *present_elts, uint64_t num_present,
                                  uint64_t groups, uint64_t chunk, int32_t *kind, uint32_t *elt, uint32_t *rounds, uint64_t *steps5,
                                  uint64_t capacity, uint64_t *count);
/* Host only, no device access: the product launches of hipbfv_batch_dot_plain_ntt_queries, 6 words per step
 * {first_query, queries, first_row, rows, QT, RT}: one launch multiplies those queries against those rows, QT queries and RT rows
 * per thread; QT == 1 names today's single-query kernel.  One query is one such step; otherwise the queries go in order, as many per
 * launch as keep ceil(rows / RT) * ceil(queries / QT) at most 2^31 - 1 (a whole number of tiles; all of them in practice), and a
 * last launch left with one query is a QT == 1 step.  Every step covers all rows.  rows == 0 or K == 0 is HIPBFV_E_INVALIDARG;
 * *count = the number of steps (E_INVALIDARG when it exceeds capacity, nothing written past it). */
long hipbfv_debug_dot_queries_plan(uint64_t queries, uint64_t rows, uint64_t K, uint64_t *steps6, uint64_t capacity,
                                   uint64_t *count);
/* Host only, no device access: the weight table of the weighted sums for the moduli `primes` (each in [2, 2^62)).
 * out[(t * count + i) * 2] = weights[t] mod primes[i], canonical; out[... + 1] = floor(that * 2^64 / primes[i]). */
long hipbfv_debug_weight_residues(const uint64_t *primes, uint64_t count, const int32_t *weights, uint64_t terms,
                                  uint64_t *out);

/* Per-kernel timing (HIP events recorded on the launch stream, around every kernel launch):
 * total milliseconds, number of launches and work units (residue polynomials for the NTT kernels,
 * polynomials or operations for the others) since the last reset. */
long hipbfv_profile_enable(void *evaluator, bool enabled);
long hipbfv_profile_reset(void *evaluator);
long hipbfv_profile_kernel_count(uint32_t *count);
long hipbfv_profile_read(void *evaluator, uint32_t kernel_id, char *name, uint64_t name_capacity, double *total_ms,
                         uint64_t *launches, uint64_t *units);

#ifdef __cplusplus
}
#endif
#endif /* HIPBFV_H */
